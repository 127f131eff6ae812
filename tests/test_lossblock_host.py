"""CPU tier of the loss-block checks: the fp64 references of tests/lossblock_ref.py tied to float64 autograd of the reference's literal
expressions (wgan_gp_loss.py:8-10,19,31,48,55,62,72-73; nn.Linear for the last layer), and the launch geometry the bounds count with."""
import numpy as np
import torch
import torch.nn.functional as F

import lossblock_ref as ref

TOL = 1e-12


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= TOL * np.maximum(np.abs(b).max(), 1e-300)))


def _rn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def test_chain_lengths_follow_the_launch_geometry():
    # terms per thread (4 per float4) + 6 shuffle levels + 4 waves + workgroups + 1: one workgroup up to 8192 floats, 256 from 2 097 152 on
    assert [ref.row_sumsq_chain(E) for E in (4, 8192, 8196, 2097152, 2097156, 3145728)] == [16, 44, 33, 299, 303, 315]
    assert [ref.gp_blocks(E) for E in (4, 1024, 1028, 1048576, 1048580, 3145728)] == [1, 1, 2, 1024, 1024, 1024]


def test_gradient_penalty_and_seed_are_autograd_of_the_norm():
    gen = torch.Generator().manual_seed(3)
    lam, inv_n = 10.0, ref.f32(1.0 / 3.0)
    for target in (1.0, 750.0):
        g = _rn(gen, 4, 48) * target / 5
        g[0] = 0                                             # zero norm: autograd's subgradient of the norm is 0, and so is the seed
        g[1] = 0
        g[1, 7] = target                                     # the norm IS the target
        g.requires_grad_(True)
        gp = ((g.norm(2, dim=1) - target) ** 2) * lam / (target ** 2)
        (gp * inv_n).sum().backward()
        ss = (g.detach() ** 2).sum(1)
        want_gp, b_gp, want_u, b_u = ref.gp_seed(g.detach().numpy(), ss.numpy(), lam, target, inv_n)
        assert _close(want_gp, gp.detach().numpy()) and _close(want_u, g.grad.numpy())
        assert want_gp[0] == lam and want_gp[1] == 0 and not want_u[:2].any() and not g.grad[:2].any()
        assert not np.isnan(b_gp).any() and not np.isnan(b_u).any() and np.all(b_gp >= 0) and np.all(b_u >= 0) and b_u[2:].min() > 0
        s, b = ref.row_sumsq(g.detach().numpy())
        assert _close(s, ss.numpy()) and np.all(b == ref.row_sumsq_chain(48) * ref.U * s * ref.WIDEN)


def test_mix_is_the_rowwise_interpolation():
    gen = torch.Generator().manual_seed(4)
    real, fake = _rn(gen, 5, 3, 4, 4), _rn(gen, 5, 3, 4, 4)
    m = torch.tensor([[0.0], [1.0], [0.375], [0.5], [0.875]], dtype=torch.float64)        # (1 - m is exact in fp32 for these)
    mul_rowwise = lambda a, b: (a.view(a.size(0), -1) * b).view(a.size())
    mixed = mul_rowwise(real, 1 - m) + mul_rowwise(fake, m)
    want, bound = ref.gp_mix(real.numpy(), fake.numpy(), m.numpy().reshape(-1))
    assert _close(want, mixed.reshape(5, -1).numpy()) and np.all(bound >= 0)
    assert np.array_equal(want[0], real[0].reshape(-1).numpy()) and np.array_equal(want[1], fake[1].reshape(-1).numpy())


def test_loss_algebra_is_autograd_of_the_reference_expressions():
    gen = torch.Generator().manual_seed(5)
    for N in (1, 3, 65, 130):
        for eps in (ref.f32(0.001), 0.0):
            scores = (_rn(gen, 3 * N) * 10 ** (torch.rand(3 * N, generator=gen, dtype=torch.float64) * 3)).requires_grad_(True)
            gp = torch.rand(N, generator=gen, dtype=torch.float64) * 10
            D_real, D_fake = scores[:N], scores[N:2 * N]
            D_real_loss = -D_real + D_real ** 2 * eps
            D_fake_loss = D_fake
            D_cost = (D_fake_loss + D_real_loss + gp).mean()
            D_cost.backward()
            want = ref.d_loss(scores.detach().numpy(), gp.numpy(), N, eps)
            assert _close(want['d_cost'][0], float(D_cost.detach())) and _close(want['d_real_loss'][0], D_real_loss.detach().numpy())
            assert np.array_equal(want['d_fake_loss'][0], D_fake.detach().numpy()) and _close(want['gscore'][0], scores.grad.numpy())
            assert not want['gscore'][0][2 * N:].any() and not want['gscore'][1][2 * N:].any() and not want['d_fake_loss'][1].any()
            assert all(np.all(np.asarray(b) >= 0) for _, b in want.values()) and want['d_cost'][1] > 0
            D = scores.detach()[:N].clone().requires_grad_(True)
            G_cost = (-D).mean()
            G_cost.backward()
            gc, b_gc, gs, b_gs = ref.g_loss(D.detach().numpy())
            assert _close(gc, float(G_cost.detach())) and _close(gs, D.grad.numpy()) and b_gc > 0 and np.all(b_gs > 0)


def test_linear1_is_nn_linear_and_its_autograd():
    gen = torch.Generator().manual_seed(6)
    for N, C in ((1, 1), (9, 65), (130, 257)):
        for slope in (ref.f32(0.2), 0.0):
            x = _rn(gen, N, C)
            x.view(-1)[::3] = 0
            x.requires_grad_(True)
            w, b = _rn(gen, 1, C).requires_grad_(True), _rn(gen, 1).requires_grad_(True)
            gs = _rn(gen, N)
            h = F.leaky_relu(x, slope)
            s = F.linear(h, w, b).view(N)
            s.backward(gs)
            want, bound = ref.linear1_fwd(h.detach().numpy(), w.detach().numpy(), b.detach().numpy())
            assert _close(want, s.detach().numpy()) and np.all(bound > 0)
            want, _ = ref.linear1_fwd(h.detach().numpy(), w.detach().numpy(), None)
            assert _close(want, F.linear(h, w).view(N).detach().numpy())
            gh, bound = ref.linear1_bwd_data(gs.numpy(), w.detach().numpy(), x.detach().numpy(), slope)      # LeakyReLU'(x): slope at x <= 0
            assert _close(gh, x.grad.numpy()) and np.all(bound >= 0)
            gh, _ = ref.linear1_bwd_data(gs.numpy(), w.detach().numpy(), None, slope)
            assert _close(gh, np.outer(gs.numpy(), w.detach().numpy()))
            dw0, db0 = _rn(gen, C), _rn(gen, 1)
            dw, b_w, db, b_b = ref.linear1_wgrad(gs.numpy(), h.detach().numpy(), dw0.numpy(), db0.numpy())
            assert _close(dw, (dw0 + w.grad.view(-1)).numpy()) and _close(db, float(db0 + b.grad)) and np.all(b_w > 0) and b_b > 0
            dw, _, db, b_b = ref.linear1_wgrad(gs.numpy(), h.detach().numpy(), dw0.numpy(), None)
            assert _close(dw, (dw0 + w.grad.view(-1)).numpy()) and db is None and b_b is None
