"""The WGAN-GP loss block and Linear(C, 1) on the device against fp64 evaluations of their contracts (tests/lossblock_ref.py: references
and derived per-element bounds), at the sizes around each kernel's launch geometry: the grid caps of ``pg_row_sumsq`` (2 097 152 floats per
row) and of ``pg_gp_mix`` / ``pg_gp_seed`` (1 048 576), the 64-wide N loops of the two loss kernels, the 64-lane and 256-thread tiles of the
linear kernels.  Every output lives inside a larger buffer whose surrounding elements must keep their bits."""
import ctypes

import numpy as np
import pytest
import torch

import lossblock_ref as ref

import pggan_amd as pg

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 8                                    # floats before and behind every output (keeps the 16-byte alignment of the float4 kernels)
E_MAX = 3145728                              # the 1024^2 image: the only production shape past the caps
SUMSQ_E = (4, 48, 1020, 1024, 1028, 2097152, 2097156, E_MAX)
GP_E = (4, 48, 1028, 1048576, 1048580, E_MAX)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).clone()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Slot(object):
    """``numel`` output floats inside a buffer of seeded noise (or of ``init``), GUARD floats on either side."""

    def __init__(self, numel, init=None):
        self.buf = torch.randn(numel + 2 * GUARD, generator=torch.Generator().manual_seed(numel)).to(DEV)
        self.out = self.buf[GUARD:GUARD + numel]
        if init is not None:
            self.out.copy_(torch.as_tensor(init, dtype=torch.float32).reshape(-1))
        self.before = _bits(self.buf)

    def ptr(self):
        return self.out.data_ptr()

    def guards_intact(self):
        now = _bits(self.buf)
        return torch.equal(now[:GUARD], self.before[:GUARD]) and torch.equal(now[-GUARD:], self.before[-GUARD:])

    def f64(self):
        return self.out.cpu().double().numpy()


def _hold(what, got, want, bound, worst):
    got, want, bound = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, bound))
    assert not np.isnan(got).any(), what
    err = np.abs(got - want)
    worst.append(float(np.max(err / np.maximum(bound, 1e-300))) if err.max() > 0 else 0.0)
    assert np.all(err <= bound), (what, int(np.argmax(err - bound)), float((err - bound).max()))


@pytest.fixture(scope='module')
def images():
    """Two seeded host tensors of 3 x E_MAX floats, randn * 10^U(-2, 1), shared and never written: every case slices rows of E floats."""
    gen = torch.Generator().manual_seed(99)
    mk = lambda: torch.randn(3 * E_MAX, generator=gen) * 10 ** (torch.rand(3 * E_MAX, generator=gen) * 3 - 2)
    return mk(), mk()


def _rows(x, N, E):
    return x[:N * E].view(N, E)


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('E', SUMSQ_E)
def test_row_sumsq(images, N, E):
    g_host = _rows(images[0], N, E)
    g = g_host.to(DEV)
    g_bits = _bits(g)
    worst = []
    for ss0 in (np.zeros(N), np.array([3.5, -1.25, 1000.0])[:N]):             # the kernel adds into what ss holds
        slot = _Slot(N, ss0)
        pg._lib.call('pg_row_sumsq', g.data_ptr(), slot.ptr(), N, E, _stream())
        torch.cuda.synchronize()
        want, bound = ref.row_sumsq(g_host.numpy(), ss0)
        _hold('ss', slot.f64(), want, bound, worst)
        assert slot.guards_intact()
    want, bound = ref.row_sumsq(g_host.numpy())
    _hold('ops.row_sumsq', pg.ops.row_sumsq(g).cpu().numpy(), want, bound, worst)                # (the wrapper zeroes first)
    assert torch.equal(_bits(g), g_bits)
    print('row_sumsq N %d E %d: chain %d, max err / bound %.3f' % (N, E, ref.row_sumsq_chain(E), max(worst)))


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('E', GP_E)
def test_gp_mix(images, N, E):
    real_h, fake_h = _rows(images[0], N, E), _rows(images[1], N, E)
    real, fake = real_h.to(DEV), fake_h.to(DEV)
    in_bits = (_bits(real), _bits(fake))
    worst = []
    for factors in ([[0.0], [1.0], [0.37]] if N == 1 else [[0.0, 1.0, 0.37], [0.618034, 0.0, 1.0]]):
        m_h = torch.tensor(factors)
        m = m_h.to(DEV)
        slot = _Slot(N * E)
        pg._lib.call('pg_gp_mix', real.data_ptr(), fake.data_ptr(), m.data_ptr(), slot.ptr(), N, E, _stream())
        torch.cuda.synchronize()
        want, bound = ref.gp_mix(real_h.numpy(), fake_h.numpy(), m_h.numpy())
        _hold('mixed', slot.f64(), want, bound, worst)
        out = slot.out.view(N, E)
        for n, f in enumerate(factors):                                          # a factor of exactly 0 or 1 selects one image exactly
            if f in (0.0, 1.0):
                assert bool((out[n] == (real if f == 0.0 else fake)[n]).all()), (n, f)
        assert slot.guards_intact()
        assert torch.equal(_bits(real), in_bits[0]) and torch.equal(_bits(fake), in_bits[1]) and torch.equal(m.cpu(), m_h)
    print('gp_mix N %d E %d (%d workgroups per row): max err / bound %.3f' % (N, E, ref.gp_blocks(E), max(worst)))


def _seed_rows(images, kinds, E, target):
    """Rows of E floats by kind: 'zero' (all zeros), 'hit' (one non-zero element equal to the target: the norm IS the target), 'plain'
    (seeded noise scaled to a norm of about 1.3 targets)."""
    g = _rows(images[0], len(kinds), E).clone()
    for n, kind in enumerate(kinds):
        if kind == 'zero':
            g[n] = 0
        elif kind == 'hit':
            g[n] = 0
            g[n, E // 3] = target
        else:
            g[n] *= 1.3 * target / float(g[n].double().norm())
    return g


@pytest.mark.parametrize('target', [1.0, 750.0])
@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('E', GP_E)
def test_gp_seed(images, N, E, target):
    lam, inv_n = 10.0, 1.0 / 3.0
    worst = []
    for kinds in ([['zero'], ['hit'], ['plain']] if N == 1 else [['zero', 'hit', 'plain']]):
        g_h = _seed_rows(images, kinds, E, target)
        ss_h = (g_h.double() ** 2).sum(1).float()                               # an operand here: exactly 0 and target^2 on the special rows
        g, ss = g_h.to(DEV), ss_h.to(DEV)
        in_bits = (_bits(g), _bits(ss))
        gp, u = _Slot(N), _Slot(N * E)
        pg._lib.call('pg_gp_seed', g.data_ptr(), ss.data_ptr(), gp.ptr(), u.ptr(), N, E, lam, target, inv_n, _stream())
        torch.cuda.synchronize()
        want_gp, b_gp, want_u, b_u = ref.gp_seed(g_h.numpy(), ss_h.numpy(), lam, target, inv_n)
        _hold('gp', gp.f64(), want_gp, b_gp, worst)
        _hold('u', u.f64(), want_u, b_u, worst)
        for n, kind in enumerate(kinds):
            row = u.out.view(N, E)[n]
            if kind == 'zero':                                                   # norm == 0: gp = lambda, and the seed is DEFINED as 0
                assert float(gp.out[n]) == lam and want_gp[n] == lam and not bool(row.any())
            elif kind == 'hit':                                                  # norm == target: no penalty, no seed
                assert float(gp.out[n]) == 0.0 and want_gp[n] == 0.0 and not bool(row.any())
            else:
                assert float(row.abs().max()) > 0
        assert gp.guards_intact() and u.guards_intact()
        assert torch.equal(_bits(g), in_bits[0]) and torch.equal(_bits(ss), in_bits[1])
    print('gp_seed N %d E %d target %g: max err / bound %.3f' % (N, E, target, max(worst)))


@pytest.mark.parametrize('eps', [0.001, 0.0])
@pytest.mark.parametrize('N', [1, 3, 64, 65, 130])
def test_d_loss_and_g_loss(N, eps):
    gen = torch.Generator().manual_seed(7 + N)
    s_h = torch.randn(3 * N, generator=gen) * 10 ** (torch.rand(3 * N, generator=gen) * 3)    # eps s^2 reaches the size of the linear term
    gp_h = torch.rand(N, generator=gen) * 10
    s, gpv = s_h.to(DEV), gp_h.to(DEV)
    in_bits = (_bits(s), _bits(gpv))
    slots = dict(d_cost=_Slot(1), d_real_loss=_Slot(N), d_fake_loss=_Slot(N), gscore=_Slot(3 * N))
    pg._lib.call('pg_d_loss', s.data_ptr(), gpv.data_ptr(), slots['d_cost'].ptr(), slots['d_real_loss'].ptr(), slots['d_fake_loss'].ptr(),
                 slots['gscore'].ptr(), N, eps, _stream())
    torch.cuda.synchronize()
    want = ref.d_loss(s_h.numpy(), gp_h.numpy(), N, eps)
    worst = []
    for name, slot in slots.items():
        _hold(name, slot.f64(), want[name][0], want[name][1], worst)
        assert slot.guards_intact(), name
    assert not bool(slots['gscore'].out[2 * N:].any())                          # the mixed third: exactly zero
    if eps and N >= 64:
        assert float(np.max(eps * np.abs(f64(s_h[:N])))) > 0.5                  # (eps s^2 against |s|: the quadratic term is of the linear one's size)
    g_cost, g_gs = _Slot(1), _Slot(N)
    pg._lib.call('pg_g_loss', s.data_ptr(), g_cost.ptr(), g_gs.ptr(), N, _stream())
    torch.cuda.synchronize()
    wc, bc, wg, bg = ref.g_loss(s_h[:N].numpy())
    _hold('g_cost', g_cost.f64(), wc, bc, worst)
    _hold('g gscore', g_gs.f64(), wg, bg, worst)
    assert g_cost.guards_intact() and g_gs.guards_intact()
    assert torch.equal(_bits(s), in_bits[0]) and torch.equal(_bits(gpv), in_bits[1])
    print('d_loss / g_loss N %d eps %g: max err / bound %.3f' % (N, eps, max(worst)))


def f64(t):
    return t.double().numpy()


@pytest.mark.parametrize('N', [1, 9, 130])
@pytest.mark.parametrize('C', [1, 63, 64, 65, 255, 256, 257, 512])
def test_linear1(N, C):
    gen = torch.Generator().manual_seed(1000 * N + C)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    h_h, w_h, b_h, gs_h, mask_h = rn(N, C), rn(C), rn(1), rn(N), rn(N, C)
    mask_h.view(-1)[::3] = 0                                                     # mask == 0 takes the slope, like mask < 0
    dw0, db0 = rn(C), rn(1)
    h, w, b, gs, mask = (x.to(DEV) for x in (h_h, w_h, b_h, gs_h, mask_h))
    in_bits = [_bits(x) for x in (h, w, b, gs, mask)]
    worst = []
    for bias in (b, None):
        slot = _Slot(N)
        pg._lib.call('pg_linear1_fwd', h.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), slot.ptr(), N, C, _stream())
        torch.cuda.synchronize()
        want, bound = ref.linear1_fwd(h_h.numpy(), w_h.numpy(), None if bias is None else b_h.numpy())
        _hold('fwd', slot.f64(), want, bound, worst)
        assert slot.guards_intact()
    for mk, slope in ((None, 0.2), (mask, 0.2), (mask, 0.0)):
        slot = _Slot(N * C)
        pg._lib.call('pg_linear1_bwd_data', gs.data_ptr(), w.data_ptr(), None if mk is None else mk.data_ptr(), slot.ptr(), N, C, slope, _stream())
        torch.cuda.synchronize()
        want, bound = ref.linear1_bwd_data(gs_h.numpy(), w_h.numpy(), None if mk is None else mask_h.numpy(), slope)
        _hold('bwd_data', slot.f64(), want, bound, worst)
        if mk is not None and slope == 0.0:
            assert not bool(slot.out.view(N, C)[mask <= 0].any())
        assert slot.guards_intact()
    for with_db in (True, False):                                                # db == nullptr: a layer without bias
        dw, db = _Slot(C, dw0), _Slot(1, db0)
        pg._lib.call('pg_linear1_wgrad', gs.data_ptr(), h.data_ptr(), dw.ptr(), db.ptr() if with_db else None, N, C, _stream())
        torch.cuda.synchronize()
        want_w, b_w, want_b, b_b = ref.linear1_wgrad(gs_h.numpy(), h_h.numpy(), dw0.numpy(), db0.numpy() if with_db else None)
        _hold('dw', dw.f64(), want_w, b_w, worst)
        if with_db:
            _hold('db', db.f64(), want_b, b_b, worst)
            assert float(np.abs(want_b - f64(db0)[0])) > 0
        else:
            assert torch.equal(_bits(db.buf), db.before)
        assert dw.guards_intact() and db.guards_intact()
    assert all(torch.equal(_bits(x), b0) for x, b0 in zip((h, w, b, gs, mask), in_bits))
    print('linear1 N %d C %d: max err / bound %.3f' % (N, C, max(worst)))
