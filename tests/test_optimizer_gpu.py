"""The optimizer step on the device: ``pg_adam`` against the fp64 evaluation of its contract at the sizes of its launch geometry, on
operands of mixed magnitude, and ``FusedAdam`` step by step against a ``torch.optim.Adam`` in float64 (tests/emu_adam.py: reference
and derived per-element bound)."""
import ctypes

import numpy as np
import pytest
import torch

import emu_adam

import pggan_amd as pg

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# 2 097 152 floats fill the capped grid (2048 x 256 threads x 4) exactly once; the last size is two full passes of it plus a 3-element
# tail and 4 more (grid-stride loop and tail)
SIZES = (1, 3, 4, 5, 1023, 1024, 2097152, 4194311)
GUARD = 8
LR, BETA2, EPS = 1e-3, 0.99, 1e-8
FULL = [(b1, gs, t) for b1 in (0.0, 0.9) for gs in (1.0, 0.125) for t in (1, 2, 1000)]
LARGE = [(0.0, 1.0, 1), (0.0, 0.125, 1000), (0.9, 0.125, 2), (0.9, 1.0, 1000)]      # both instantiations, both scales, all three steps


def _bits(t):
    return t.detach().cpu().view(torch.int32).clone()


@pytest.fixture(scope='module')
def operands():
    """Seeded host operands of the largest size (+ the guard elements), shared and never written; every case slices them.
    p = randn * 10^U(-3, 0.5), g = randn * 10^U(-10, 2), m = randn at g's scale, v = (randn at g's scale)^2 and 0 on a third of the
    elements.  Element i with i % 5 == 1 has v = 0 and |g| in 1e-9 .. 1e-7 (sqrt(v') is of eps's size: eps decides the step); with
    i % 5 == 2 it has g = m = v = 0 (p must keep its bits)."""
    gen = torch.Generator().manual_seed(4321)
    n = max(SIZES) + GUARD
    rn = lambda: torch.randn(n, generator=gen, dtype=torch.float64)
    un = lambda lo, hi: torch.rand(n, generator=gen, dtype=torch.float64) * (hi - lo) + lo
    p = rn() * 10 ** un(-3, 0.5)
    scale = 10 ** un(-10, 2)
    g, m, v = rn() * scale, rn() * scale, (rn() * scale) ** 2
    i = torch.arange(n)
    v[i % 3 == 0] = 0
    tiny = i % 5 == 1
    g[tiny] = torch.where(g[tiny] < 0, -1.0, 1.0) * 10 ** un(-9, -7)[tiny]
    v[tiny] = 0
    zero = i % 5 == 2
    g[zero], m[zero], v[zero] = 0, 0, 0
    return tuple(x.float() for x in (p, g, m, v))


@pytest.mark.parametrize('n', SIZES)
def test_kernel_against_fp64(operands, n):
    p0, g0, m0, v0 = (x[:n + GUARD].to(DEV) for x in operands)
    g0 = g0[:n].clone()
    p64, g64, m64, v64 = (x[:n].double().numpy() for x in operands)
    g_bits = _bits(g0)
    if n >= 3:
        tiny, zero = np.arange(n) % 5 == 1, np.arange(n) % 5 == 2
        assert tiny.any() and zero.any() and np.all(v64[tiny] == 0) and np.all((np.abs(g64[tiny]) >= 1e-9) & (np.abs(g64[tiny]) <= 1e-7))
        assert np.all(g64[zero] == 0) and np.all(v64[zero] == 0) and np.all(m64[zero] == 0)
    for beta1, gs, t in (FULL if n <= 1024 else LARGE):
        bc1, bc2s = emu_adam.bias_corrections(t, beta1, BETA2)
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        if beta1 == 0.0:
            m.fill_(float('nan'))                       # this instantiation never reads the old moment: a NaN there must not leak
        m_start = _bits(m)
        pg.ops.adam(p[:n], g0, m[:n], v[:n], LR, beta1, BETA2, EPS, bc1, bc2s, gs)
        torch.cuda.synchronize()
        want = emu_adam.reference(p64, g64, m64, v64, LR, beta1, BETA2, EPS, bc1, bc2s, gs)
        ratios = []
        for name, got, ref, bound in zip('pmv', (p, m, v), want[:3], want[3:]):
            got = got[:n].cpu().double().numpy()
            assert not np.isnan(got).any(), (name, n, beta1, gs, t)
            err = np.abs(got - ref)
            ratios.append(float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (name, n, beta1, gs, t, int(np.argmax(err - bound)), float((err - bound).max()))
        print('n %d beta1 %g grad_scale %g step %d: max err / bound p %.3f m %.3f v %.3f' % ((n, beta1, gs, t) + tuple(ratios)))
        if beta1 == 0.0:                                # FusedAdam.flat_moments: m is exactly the last gradient x grad_scale
            assert bool((m[:n] == g0 * gs).all())
        if n >= 3:                                      # g == 0 and v == 0 (and m == 0): nothing moves
            sel = torch.from_numpy(zero)
            assert torch.equal(_bits(p[:n])[sel], _bits(p0[:n])[sel])
        # the eight elements behind each range, and the gradient
        assert torch.equal(_bits(p[n:]), _bits(p0[n:])) and torch.equal(_bits(m[n:]), m_start[n:]) and torch.equal(_bits(v[n:]), _bits(v0[n:]))
        assert torch.equal(_bits(g0), g_bits)


def test_argument_errors_launch_nothing():
    bufs = [torch.randn(64, device=DEV) for _ in range(4)]
    before = [_bits(b) for b in bufs]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = [b.data_ptr() for b in bufs]
    tail = (1e-3, 0.9, 0.99, 1e-8, 0.1, 0.1, 1.0, s)
    cases = [((ptrs[0], ptrs[1], ptrs[2], ptrs[3], 0), 'PG_E_ARG')]
    for i in range(4):
        null, off = list(ptrs), list(ptrs)
        null[i], off[i] = None, ptrs[i] + 4
        cases += [(tuple(null) + (32,), 'PG_E_ARG'), (tuple(off) + (32,), 'PG_E_ALIGN')]
    for args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            pg._lib.call('pg_adam', *(args + tail))
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(b), b0) for b, b0 in zip(bufs, before))


def _f64(t):
    return t.detach().cpu().double()


def test_fused_adam_against_float64_twin():
    """Three D steps of the narrow 8x8 pair at depth 1 (the 4x4-stage fromRGB layer has no gradient).  Before every step the parameters,
    their gradients and the flat moments are copied to the host; a ``torch.optim.Adam`` in float64 whose state holds those copies, with
    its OWN per-parameter step counter, takes the same step.  That isolates the optimizer from the gradients and pins the step counts:
    ``emu_adam.reference`` with the twin's count must agree with the twin up to the rounding of the scalars to fp32, and the device
    must agree with that reference within the kernel's bound."""
    torch.manual_seed(1)
    D = pg.Discriminator((1, 3, 8, 8), fmap_base=64, fmap_max=16).to(DEV)
    G = pg.Generator((1, 3, 8, 8), fmap_base=64, fmap_max=16, latent_size=16).to(DEV)
    D.depth = G.depth = 1
    opt = pg.FusedAdam(D.parameters(), LR, betas=(0.0, BETA2))
    real, z = torch.rand(4, 3, 8, 8, device=DEV), torch.randn(4, 16, device=DEV)
    names = [k for k, _ in D.named_parameters()]
    params = [q for _, q in D.named_parameters()]
    base = D._flat_param.data_ptr()
    spans = [((q.data_ptr() - base) // 4, q.numel()) for q in params]
    covered = torch.zeros(D._flat_param.numel(), dtype=torch.bool)
    for off, cnt in spans:
        covered[off:off + cnt] = True
    assert bool((~covered).any())                                         # there IS padding between parameters
    twin_params = [torch.nn.Parameter(torch.zeros(q.shape, dtype=torch.float64)) for q in params]
    twin = torch.optim.Adam(twin_params, LR, betas=(0.0, BETA2), eps=EPS)
    # what the rounding of the scalars to fp32 may put between the twin (Python-float scalars) and the reference (fp32 scalars):
    # 1 - fp32(beta2) against 1 - beta2 on v' and, through sqrt(v') and the bias correction, half of it each on the step; 8u for
    # lr, bc1, their quotient, bc2_sqrt, its reciprocal and eps
    r_omb2 = abs(float(np.float32(1) - np.float32(BETA2)) - (1.0 - BETA2)) / (1.0 - BETA2)
    launches = []
    hook = lambda fn, args, name: (launches.append(name), fn(*args))[1]
    pad_start = _bits(D._flat_param)[~covered]
    for it in range(3):
        pg.wgan_gp_loss.set_mixing_factors(torch.full((4, 1), 0.25 + 0.25 * it))
        c, _, _ = pg.wgan_gp_D_loss(D, G, real, z)
        c.backward()
        torch.cuda.synchronize()
        mom = opt.flat_moments(D)
        assert (mom is None) == (it == 0)
        m_flat = _f64(mom[0]) if mom else torch.zeros(covered.numel(), dtype=torch.float64)
        v_flat = _f64(mom[1]) if mom else torch.zeros(covered.numel(), dtype=torch.float64)
        before_bits = _bits(D._flat_param)
        active = [q.grad is not None for q in params]
        assert any(active) and not all(active)
        for q, tq, (off, cnt) in zip(params, twin_params, spans):
            tq.data.copy_(_f64(q))
            tq.grad = None if q.grad is None else _f64(q.grad).reshape(q.shape).clone()
            if tq in twin.state and twin.state[tq]:
                twin.state[tq]['exp_avg'].copy_(m_flat[off:off + cnt].view(q.shape))
                twin.state[tq]['exp_avg_sq'].copy_(v_flat[off:off + cnt].view(q.shape))
        start = [(tq.data.clone(), None if tq.grad is None else tq.grad.clone()) for tq in twin_params]
        # contiguous runs of parameters with a gradient (same step count here: the active set does not change at a fixed depth)
        runs, end = 0, None
        for (off, cnt), a in sorted(zip(spans, active)):
            if a:
                runs += off != end
                end = off + (cnt + 3) // 4 * 4
        twin.step()
        del launches[:]
        pg._lib.CALL_HOOK = hook
        try:
            opt.step()
        finally:
            pg._lib.CALL_HOOK = None
        torch.cuda.synchronize()
        assert launches.count('pg_adam') == runs and runs >= 1, (launches, runs)
        m_dev, v_dev = (_f64(x) for x in opt.flat_moments(D))
        after = _f64(D._flat_param)
        after_bits = _bits(D._flat_param)
        worst = 0.0
        for name, q, tq, (off, cnt), a, (p_start, g_start) in zip(names, params, twin_params, spans, active, start):
            sl = slice(off, off + cnt)
            if not a:
                assert torch.equal(after_bits[sl], before_bits[sl]), name              # no gradient: the bits stay
                assert not bool(m_dev[sl].any()) and not bool(v_dev[sl].any()), name   # ... and the moments stay zero
                assert not twin.state[tq]
                continue
            t = int(twin.state[tq]['step'])
            assert t == it + 1
            bc1, bc2s = emu_adam.bias_corrections(t, 0.0, BETA2)
            rp, rm, rv, bp, bm, bv = emu_adam.reference(p_start.reshape(-1).numpy(), g_start.reshape(-1).numpy(), m_flat[sl].numpy(),
                                                        v_flat[sl].numpy(), LR, 0.0, BETA2, EPS, bc1, bc2s, 1.0)
            q_abs = np.abs(rp - p_start.reshape(-1).numpy())
            tp, tm, tv = (x.reshape(-1).numpy() for x in (tq.data, twin.state[tq]['exp_avg'], twin.state[tq]['exp_avg_sq']))
            assert np.all(np.abs(rp - tp) <= (r_omb2 + 8 * emu_adam.U) * q_abs + 2.0 ** -52 * np.abs(tp)), name
            assert np.all(np.abs(rv - tv) <= (r_omb2 + 2 * emu_adam.U) * tv) and np.array_equal(rm, tm), name
            for what, got, ref, bound in (('p', after[sl], rp, bp), ('m', m_dev[sl], rm, bm), ('v', v_dev[sl], rv, bv)):
                err = np.abs(got.numpy() - ref)
                worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
                assert np.all(err <= bound), (it, name, what, float((err - bound).max()))
            assert q_abs.max() > 1e-5                                                  # the step is there to be seen
        print('FusedAdam step %d: %d launches, max err / bound %.3f' % (it + 1, runs, worst))
        # the padding between parameters, which a merged launch runs over: zero gradient, zero moments -> stays exactly zero
        assert torch.equal(after_bits[~covered], pad_start) and not bool(pad_start.any())
        assert not bool(m_dev[~covered].any()) and not bool(v_dev[~covered].any())
