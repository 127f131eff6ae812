"""CPU tier of the optimizer checks: the fp64 reference of one ``pg_adam`` step (tests/emu_adam.py) tied to ``torch.optim.Adam`` in float64,
and a proof that the movement assertion of the trainer trace (helpers.trace_movement_errors) sees a step that is 2 % too long."""
import numpy as np
import pytest
import torch

import emu_adam
import emu_ops
from helpers import TRACE_MOVEMENT_TOL_HOST, trace_movement_errors
from test_engine_host import emu, run_trainer_trace  # noqa: F401  (the fixture)

LR, EPS = 1e-3, 1e-8


def _operands(n=4099):
    gen = torch.Generator().manual_seed(17)
    p = torch.randn(n, generator=gen, dtype=torch.float64) * 10 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 3.5 - 3)
    grads = [torch.randn(n, generator=gen, dtype=torch.float64) * 10 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 12 - 10)
             for _ in range(3)]
    return p, grads


@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
@pytest.mark.parametrize('beta1', [0.0, 0.9])
def test_reference_is_torch_adam_in_float64(beta1, grad_scale):
    """Three steps from zero moments, the step counts and bias corrections formed as ``FusedAdam.step`` forms them; the scalars are taken
    exactly (``exact=True``), so that what is compared is the formula.  ``torch.optim.Adam`` is the reference's optimizer
    (betas (0.0, 0.99); beta1 = 0.9 for the other instantiation)."""
    beta2 = 0.99
    p0, grads = _operands()
    tp = torch.nn.Parameter(p0.clone())
    twin = torch.optim.Adam([tp], LR, betas=(beta1, beta2), eps=EPS)
    p, m, v = p0.numpy().copy(), np.zeros(p0.numel()), np.zeros(p0.numel())
    for t, g in enumerate(grads, 1):
        tp.grad = g * grad_scale
        twin.step()
        bc1, bc2s = emu_adam.bias_corrections(t, beta1, beta2)
        before = p
        p, m, v, bp, bm, bv = emu_adam.reference(p, g.numpy(), m, v, LR, beta1, beta2, EPS, bc1, bc2s, grad_scale, exact=True)
        st = twin.state[tp]
        assert int(st['step']) == t
        step = np.abs(p - before)
        assert np.all(np.abs(p - tp.detach().numpy()) <= 1e-12 * (np.abs(before) + step))
        assert np.all(np.abs(m - st['exp_avg'].numpy()) <= 1e-12 * np.abs(m))
        assert np.all(np.abs(v - st['exp_avg_sq'].numpy()) <= 1e-12 * v)
        assert all(np.all(b >= 0) and np.all(np.isfinite(b)) for b in (bp, bm, bv)) and step.max() > 1e-4


@pytest.mark.parametrize('beta1', [0.0, 0.9])
def test_fp32_scalars_stay_next_to_the_exact_ones(beta1):
    """The reference the device is held to rounds the scalars to fp32 as the C ABI does.  That moves the step by no more than the rounding
    of 1 - fp32(beta) against 1 - beta (9.5e-7 for beta2 = 0.99) plus a few 2^-24: a typo in ``scalars`` would be far outside."""
    beta2 = 0.99
    p0, grads = _operands()
    g = grads[0].numpy()
    m0, v0 = grads[1].numpy() * (beta1 != 0), grads[2].numpy() ** 2
    for t in (1, 2, 1000):
        bc1, bc2s = emu_adam.bias_corrections(t, beta1, beta2)
        a = emu_adam.reference(p0.numpy(), g, m0, v0, LR, beta1, beta2, EPS, bc1, bc2s, 0.125)
        b = emu_adam.reference(p0.numpy(), g, m0, v0, LR, beta1, beta2, EPS, bc1, bc2s, 0.125, exact=True)
        r = max(abs(float(np.float32(1) - np.float32(x)) - (1.0 - x)) / (1.0 - x) for x in (beta1, beta2))
        r += abs(float(np.float32(beta1)) - beta1) + abs(float(np.float32(beta2)) - beta2)
        q = np.abs(b[0] - p0.numpy())
        assert np.all(np.abs(a[0] - b[0]) <= (2 * r + 8 * emu_adam.U) * (q + LR / bc1 * np.abs(m0) / (np.sqrt(b[2]) / bc2s + EPS))
                      + 2.0 ** -51 * np.abs(p0.numpy()))           # (q is read off p' - p in fp64)
        assert np.all(np.abs(a[2] - b[2]) <= (r + 2 * emu_adam.U) * b[2])
        assert np.all(np.abs(a[1] - b[1]) <= (r + 2 * emu_adam.U) * (np.abs(m0) + np.abs(g)))


def test_zero_gradient_and_zero_moments_leave_the_parameter():
    p = np.float64([1.5, -2.25e-3, 0.0])
    z = np.zeros(3)
    for beta1 in (0.0, 0.9):
        p1, m1, v1, bp, bm, bv = emu_adam.reference(p, z, z, z, LR, beta1, 0.99, EPS, 0.1, 0.1)
        assert np.array_equal(p1, p) and not m1.any() and not v1.any() and not np.isnan(bp).any()
        assert np.all(bp <= emu_adam.U * np.abs(p) * emu_adam.SECOND_ORDER) and not bm.any() and not bv.any()


def test_trace_movement_sees_a_two_percent_step(emu, monkeypatch):
    """The same 14 iterations as ``test_trainer_trace`` with the learning rate of every Adam launch scaled by 1.02 -- here, in the test's
    own wrapper, and nowhere else.  Every tensor the fixture moved must then miss the host bound (measured: 1.96e-2 at the least, against
    2e-4); the weight assertion of the trace (rel. max-norm 2e-3) reads 1e-4 for the same run and passes."""
    plain = emu_ops.adam

    def long_step(p, g, m, v, lr, *rest, **kw):
        return plain(p, g, m, v, lr * 1.02, *rest, **kw)
    monkeypatch.setattr(emu_ops, 'adam', long_step)
    meta, data, G, D = run_trainer_trace(check_losses=False)
    moved = trace_movement_errors(data, G=G, D=D)
    print('movement with a 1.02 step: min %.2e, max %.2e over %d tensors' % (min(moved.values()), max(moved.values()), len(moved)))
    assert len(moved) >= 20 and min(moved.values()) > TRACE_MOVEMENT_TOL_HOST, moved
    assert min(moved.values()) > 1e-2                        # (a 2 % step reads about 2e-2: the GPU tier's bound may not exceed 1e-2)
