"""Every kernel family once, inside guard bands (tests/redzone.py, docs/experiments_redzone.md), on the MI355X.

Each test makes the call and the tests/emu_ops.py comparison of the per-kernel tiers (test_kernels_gpu.py, test_winograd.py,
test_strip_gpu.py) at their tolerances -- 2e-5, 5e-5 for weight gradients, 1e-4 for the mbstd tangent / HVP terms -- but every
input is a ``guard``ed view (16-byte aligned and no better, NaN / +-1 / 0xFF / 0x00 on either side), every output the wrappers
allocate comes from the recording allocator, and every call is followed by ``check``: bands intact, inputs unchanged, outputs
fully written.  Shapes are the smallest ragged ones, square and -- the C-ABI takes H and W separately -- W > H and H > W.
The last test asserts that every conv kernel family was launched under the guards, so the module is meant to run whole."""
import ctypes

import pytest
import torch

import emu_ops as E
from conftest import rel_err
from philox_ref import _philox4x32_10
from redzone import POLARITIES, Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops
TOL, TOL_WGRAD, TOL_HVP = 2e-5, 5e-5, 1e-4
SEEN = set()                                                  # kernel families (text before '<') launched under the guards

# Outputs a header documents as possibly unwritten (include/pggan_hip.h), by '<wrapper>:<ordinal of its allocation>':
#   pg_conv2d_pool_nhwc: "y = act(conv) ... (left UNWRITTEN when pool_only != 0 and the fused path is taken; always pass a valid buffer)"
#   pg_conv2d_wino_nhwc: "with the optional fused epilogues of pg_conv2d_pool_nhwc (ypool/pool_other/pool_a/pool_b/pool_only)" (pool_only form)
POOL_ONLY_Y = ('conv2d_pool:0', 'conv2d_wino:0')
#   pg_conv2d_unpool_nhwc: "`y` ([N][Hout][Wout][Cout]) is scratch: written only when the launch cannot fuse (split-K / small-M / thin kernels)"
UNPOOL_SCRATCH_Y = ('conv2d_unpool:0',)
#   pg_mbstd_fwd: "stats: G rows of PG_MBSTD_STATS_STRIDE floats, row g = {mu, sigma, workspace of the multi-workgroup reduction...}":
#   only mu and sigma are results, how much of the workspace a launch uses is its own business
MBSTD_STATS = ('mbstd_fwd:1', 'mbstd_tangent:1', 'mbstd_stats:0', 'mbstd_tangent_stats:0')


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    # test-side seam: ops.py's own torch.empty / empty_like / zeros (also _empty, Arena); every site there passes device= of an input
    monkeypatch.setattr(ops, 'torch', r.proxy(helpers=(ops._empty, ops.Arena.take)))
    lib = pg._lib.load()
    yield r
    r.forget()
    for key in (0, 1, 2, 3):
        lib.pg_debug_set_tuning(key, -1)
    lib.pg_debug_set_wino(0)
    lib.pg_debug_set_wino_ksplit(-1)


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g)


def note_kernels():
    lib = pg._lib.load()
    for fn in (lib.pg_debug_last_conv_kernel, lib.pg_debug_last_wino_kernel, lib.pg_debug_last_wino_wgrad_kernel):
        name = fn().decode()
        if name:
            SEEN.add(name.split('<')[0])


def launched(before):
    """Kernel families first seen since ``before = set(SEEN)`` plus the three last-kernel names of this thread: what THIS test ran."""
    lib = pg._lib.load()
    last = set(fn().decode().split('<')[0] for fn in (lib.pg_debug_last_conv_kernel, lib.pg_debug_last_wino_kernel, lib.pg_debug_last_wino_wgrad_kernel))
    return (SEEN - before) | last


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)
    note_kernels()


def ok(name, got, ref, tol=TOL):
    e = rel_err(got, ref)
    print('%-70s rel_err %.2e' % (name, e))
    assert e < tol, (name, e)                                  # (NaN from a band: not < tol)


def refused(rz, fn):
    """fn() or None when the dispatcher refuses (ops.Unsupported: the caller keeps a path that works)."""
    try:
        return fn()
    except ops.Unsupported:
        rz.discard_outputs()
        return None


class tuning(object):
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        assert pg._lib.load().pg_debug_set_tuning(self.key, self.value) == 0

    def __exit__(self, *exc):
        pg._lib.load().pg_debug_set_tuning(self.key, -1)
        return False


# ------------------------------------------------------------------------------------------------- direct conv
def conv_case(rz, N, H, W, ci, co, ks, pad, ups, wgrad=True, may_refuse=False):
    G = rz.guard
    hin, win = (H // 2, W // 2) if ups else (H, W)
    ho, wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    x, w, b = rnd(N, hin, win, ci), rnd(ks, ks, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    m = rnd(N, ho, wo, co, seed=3)
    tag = str((N, H, W, ci, co, ks, pad, ups))
    xd, wd, bd = G(x, name='x'), G(w, name='w'), G(b, name='bias')
    ref = E.conv2d(x, w, b, N, H, W, ks, pad, 0.37, slope=0.2, ups=bool(ups))
    refm = E.conv2d(x, w, None, N, H, W, ks, pad, 0.37, mask=m, mask_slope=0.2, ups=bool(ups))
    if may_refuse:                                             # non-square maps only: a dispatcher may refuse instead of being taught them
        y = refused(rz, lambda: ops.conv2d(xd, wd, bd, N, H, W, ks, pad, 0.37, slope=0.2, ups=bool(ups)))
        if y is None:
            return False
    else:
        y = ops.conv2d(xd, wd, bd, N, H, W, ks, pad, 0.37, slope=0.2, ups=bool(ups))
    chk(rz)
    ok('conv fwd ' + tag, y, ref)
    for pol in POLARITIES:
        y = ops.conv2d(xd, wd, None, N, H, W, ks, pad, 0.37, mask=G(m, 'mask', pol, name='mask'), mask_slope=0.2, ups=bool(ups))
        chk(rz)
        ok('conv masked fp32 %+d %s' % (pol, tag), y, refm)
        mb = G(E.signbytes_of(m), 'mask', pol, name='mask bytes')
        y = refused(rz, lambda: ops.conv2d(xd, wd, None, N, H, W, ks, pad, 0.37, mask=mb, mask_slope=0.2, ups=bool(ups)))
        if y is not None:
            chk(rz)
            ok('conv masked bytes %+d %s' % (pol, tag), y, refm)
    out = refused(rz, lambda: ops.conv2d(xd, wd, bd, N, H, W, ks, pad, 0.37, slope=0.2, ups=bool(ups), signs_out=True))
    if out is not None:
        chk(rz)
        ok('conv signs_out y ' + tag, out[0], ref)
        assert torch.equal(out[1].cpu(), E.signbytes_of(out[0].cpu()))
    if not wgrad:
        return True
    gz = rnd(N, ho, wo, co, seed=5)
    dw0, db0 = rnd(ks, ks, co, ci, seed=6), rnd(co, seed=7)
    rw, rb = dw0.clone(), db0.clone()
    E.conv2d_wgrad(x, gz, rw, rb, N, H, W, ks, pad, 0.41, ups=bool(ups))
    gzd = G(gz, name='gz')
    for with_db in (True, False):
        dw, db = G(dw0, 'acc', name='dw'), G(db0, 'acc', name='db') if with_db else None
        ops.conv2d_wgrad(xd, gzd, dw, db, N, H, W, ks, pad, 0.41, ups=bool(ups))
        chk(rz)
        ok('wgrad dw db=%s %s' % (with_db, tag), dw, rw, TOL_WGRAD)
        if with_db:
            ok('wgrad db ' + tag, db, rb, TOL_WGRAD)
    return True


CONV_CASES = [(3, 16, 128, 96, 3, 1, 0), (2, 16, 12, 20, 3, 1, 0), (5, 4, 32, 16, 3, 1, 0), (2, 4, 8, 8, 3, 1, 0), (7, 4, 16, 16, 4, 0, 0),
              (9, 4, 80, 32, 4, 0, 0), (6, 1, 16, 32, 4, 3, 0), (33, 1, 128, 48, 4, 3, 0), (2, 16, 32, 32, 1, 0, 0), (3, 8, 64, 32, 3, 1, 1),
              (1, 16, 144, 32, 3, 1, 0), (1, 64, 8, 8, 3, 1, 0), (2, 64, 16, 8, 3, 1, 1), (1, 64, 8, 16, 3, 1, 0)]


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv2d_and_wgrad(rz, case):
    N, H, ci, co, ks, pad, ups = case
    conv_case(rz, N, H, H, ci, co, ks, pad, ups)


def test_byte_masks_on_deep_small_maps_are_served_by_the_tile_kernel(rz):
    """Cin >= 128 and at most 576 output pixels: fp32-mask launches take conv_ksplit_kernel, whose epilogue knows fp32 masks only;
    sign-byte launches must not (they once did, and read the byte array as floats).  With few (tile, cout block) pairs the generic
    tile kernel would split K itself and refuses byte masks (PG_E_UNSUP: the caller redoes the layer with fp32 masks); with >= 192
    pairs it serves them.  The shapes below have 9 x 8 x 8 = 576 pixels and 512 / 1024 couts: at least one must be SERVED, and
    every one that is must be right, in both band polarities."""
    lib = pg._lib.load()
    served = []
    for (N, H, ci, co) in ((9, 8, 128, 512), (9, 8, 128, 1024), (9, 8, 256, 1024)):
        x, w, m = rnd(N, H, H, ci), rnd(3, 3, co, ci, seed=1) * 0.2, rnd(N, H, H, co, seed=3)
        xd, wd = rz.guard(x), rz.guard(w)
        ref = E.conv2d(x, w, None, N, H, H, 3, 1, 0.37, mask=m, mask_slope=0.2)
        y = ops.conv2d(xd, wd, None, N, H, H, 3, 1, 0.37, mask=rz.guard(m, 'mask', 1), mask_slope=0.2)
        assert lib.pg_debug_last_conv_kernel().decode().startswith('conv_ksplit_kernel')        # the fp32 mask does take the small-map split
        chk(rz)
        ok('fp32 mask, small-map split %s' % ((N, H, ci, co),), y, ref)
        for pol in POLARITIES:
            mb = rz.guard(E.signbytes_of(m), 'mask', pol)
            y = refused(rz, lambda: ops.conv2d(xd, wd, None, N, H, H, 3, 1, 0.37, mask=mb, mask_slope=0.2))
            if y is not None:
                assert lib.pg_debug_last_conv_kernel().decode().startswith('conv_igemm_kernel')
                chk(rz)
                ok('byte mask %+d %s' % (pol, (N, H, ci, co)), y, ref)
                served.append((N, H, ci, co, pol))
        rz.forget()
    print('served:', served)
    assert served, 'every byte-mask launch was refused: the fixed dispatcher branch is not exercised with a result'


def test_conv_4x4_to_1x1_split_and_one_workgroup(rz):
    N, ci, co = 9, 80, 32
    lib = pg._lib.load()
    x, w, b = rnd(N, 4, 4, ci), rnd(4, 4, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    xd, wd, bd = rz.guard(x), rz.guard(w), rz.guard(b)
    ref = E.conv2d(x, w, b, N, 4, 4, 4, 0, 0.37, slope=0.2)
    y = ops.conv2d(xd, wd, bd, N, 4, 4, 4, 0, 0.37, slope=0.2)
    assert lib.pg_debug_last_conv_kernel().decode().startswith('conv_k4_reduce_split_kernel')
    chk(rz)
    ok('4x4 -> 1x1 split', y, ref)
    with tuning(3, 21):
        y = ops.conv2d(xd, wd, bd, N, 4, 4, 4, 0, 0.37, slope=0.2)
        assert lib.pg_debug_last_conv_kernel().decode().startswith('conv_k4_reduce_kernel')
        chk(rz)
    ok('4x4 -> 1x1 one workgroup', y, ref)


# ------------------------------------------------------------------------------------------- fused epilogues
def pool_case(rz, N, H, W, ci, co, cand):
    G = rz.guard
    lib = pg._lib.load()
    x, w, b = rnd(N, H, W, ci), rnd(3, 3, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    other, m = rnd(N, H // 2, W // 2, co, seed=4), rnd(N, H, W, co, seed=3)
    xd, wd, bd, od = G(x), G(w), G(b), G(other)
    ry, ryp = E.conv2d_pool(x, w, b, N, H, W, 3, 1, 0.37, slope=0.2, other=other, a=0.6, b=0.4)
    _, rtp = E.conv2d_pool(x, w, None, N, H, W, 3, 1, 0.37, mask=m, mask_slope=0.2)
    lib.pg_debug_set_tuning(0, cand)
    try:
        y, yp = ops.conv2d_pool(xd, wd, bd, N, H, W, 3, 1, 0.37, slope=0.2, other=od, a=0.6, b=0.4)
    except RuntimeError:                                       # tile candidate not available for this shape (as test_kernels_gpu.py)
        rz.discard_outputs()
        return False
    chk(rz)
    ok('conv+pool y', y, ry)
    ok('conv+pool ypool', yp, ryp)
    for pol in POLARITIES:
        _, yp2 = ops.conv2d_pool(xd, wd, None, N, H, W, 3, 1, 0.37, mask=G(m, 'mask', pol), mask_slope=0.2, pool_only=True)
        chk(rz, may_stay_unwritten=POOL_ONLY_Y)
        ok('conv+pool masked, pooled only %+d' % pol, yp2, rtp)
    return True


def unpool_case(rz, N, H, W, ci, co, cand):
    G = rz.guard
    lib = pg._lib.load()
    x, w = rnd(N, H, W, ci), rnd(3, 3, co, ci, seed=1) * 0.2
    m = rnd(N, 2 * H, 2 * W, co, seed=3)
    xd, wd = G(x), G(w)
    lib.pg_debug_set_tuning(0, cand)
    try:
        up2 = ops.conv2d_unpool(xd, wd, N, H, W, 3, 1, 0.37)
    except RuntimeError:
        rz.discard_outputs()
        return False
    chk(rz, may_stay_unwritten=UNPOOL_SCRATCH_Y)
    ok('conv+unpool (no mask)', up2, E.conv2d_unpool(x, w, N, H, W, 3, 1, 0.37))
    ref = E.conv2d_unpool(x, w, N, H, W, 3, 1, 0.37, upmask=m, mul=0.7, mask_slope=0.2)
    for pol in POLARITIES:
        up = ops.conv2d_unpool(xd, wd, N, H, W, 3, 1, 0.37, upmask=G(m, 'mask', pol), mul=0.7, mask_slope=0.2)
        chk(rz, may_stay_unwritten=UNPOOL_SCRATCH_Y)
        ok('conv+unpool fp32 mask %+d' % pol, up, ref)
        umb = G(E.signbytes_of(m), 'mask', pol)
        up = refused(rz, lambda: ops.conv2d_unpool(xd, wd, N, H, W, 3, 1, 0.37, upmask=umb, mul=0.7, mask_slope=0.2))
        if up is not None:
            chk(rz, may_stay_unwritten=UNPOOL_SCRATCH_Y)
            ok('conv+unpool byte mask %+d' % pol, up, ref)
    return True


POOL_CASES = [(2, 16, 12, 20), (5, 4, 32, 16), (2, 2, 16, 16), (1, 64, 8, 16)]
CANDS = [-1, 0, 1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize('case', POOL_CASES)
@pytest.mark.parametrize('cand', CANDS)
def test_conv2d_pool(rz, case, cand):
    N, H, ci, co = case
    if not pool_case(rz, N, H, H, ci, co, cand):
        pytest.skip('tile candidate not available for this shape')


@pytest.mark.parametrize('case', POOL_CASES)
@pytest.mark.parametrize('cand', CANDS)
def test_conv2d_unpool(rz, case, cand):
    N, H, ci, co = case
    if not unpool_case(rz, N, H, H, ci, co, cand):
        pytest.skip('tile candidate not available for this shape')


def pixelnorm_conv_case(rz, N, H, W, ci, co):
    G = rz.guard
    x, w, b = rnd(N, H, W, ci), rnd(3, 3, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    xd, wd = G(x), G(w)
    y, r = ops.conv2d_pixelnorm(xd, wd, G(b), N, H, W, 3, 1, 0.37, 0.2, 1e-8)
    chk(rz)
    ry, rr = E.conv2d_pixelnorm(x, w, b, N, H, W, 3, 1, 0.37, 0.2, 1e-8)
    ok('conv+pixelnorm y', y, ry)
    ok('conv+pixelnorm r', r, rr)
    h = rnd(N, H, W, co, seed=4)
    ys, rs = E.pixelnorm_fwd(h)
    for with_r in (True, False):
        yy, rr_ = (ys, rs) if with_r else (h, None)
        for kind, pol in (('data', 1), ('mask', 1), ('mask', -1)):
            out = ops.conv2d_pnbwd(xd, wd, G(yy, kind, pol), G(rr_), N, H, W, 3, 1, 0.37, 0.2)
            chk(rz)
            # (ysaved enters as data AND through ysaved > 0: NaN bands for the one, +-1 for the other)
            ok('conv+pnbwd r=%s %s%+d' % (with_r, kind, pol), out, E.conv2d_pnbwd(x, w, yy, rr_, N, H, W, 3, 1, 0.37, 0.2), TOL_WGRAD)


@pytest.mark.parametrize('case', [(2, 16, 12, 20), (5, 4, 32, 16), (1, 64, 8, 8)])
def test_conv2d_pixelnorm_and_pnbwd(rz, case):
    N, H, ci, co = case
    pixelnorm_conv_case(rz, N, H, H, ci, co)


def unpooled_case(rz, N, H, W, cg, co):
    G = rz.guard
    g, a2 = rnd(N, H // 2, W // 2, cg), rnd(N, H, W, cg, seed=1)
    wt, a1 = rnd(3, 3, co, cg, seed=2) * 0.2, rnd(N, H, W, co, seed=3)
    gz2 = E.avgpool2_bwd(g, a2, 0.7, 0.2)
    ref = E.conv2d(gz2, wt, None, N, H, W, 3, 1, 0.3, mask=a1, mask_slope=0.2)
    dw0, db0 = rnd(3, 3, cg, co, seed=4), rnd(cg, seed=5)
    rdw, rdb = dw0.clone(), db0.clone()
    E.conv2d_wgrad(a1, gz2, rdw, rdb, N, H, W, 3, 1, 0.41)
    gd, wtd, a1d = G(g), G(wt), G(a1)
    ran = False
    for pol in POLARITIES:
        gb = G(E.signbytes_of(a2), 'mask', pol, name='gbytes')
        for mask in (G(E.signbytes_of(a1), 'mask', pol), G(a1, 'mask', pol)):
            y = refused(rz, lambda: ops.conv2d_unpooled(gd, wtd, gb, 0.25 * 0.7, 0.2, N, H, W, 0.3, mask=mask, mask_slope=0.2))
            if y is not None:
                chk(rz)
                ok('conv of the pool adjoint %+d' % pol, y, ref)
                ran = True
        dw, db = G(dw0, 'acc'), G(db0, 'acc')
        if refused(rz, lambda: ops.conv2d_wgrad_unpooled(a1d, gd, gb, 0.25 * 0.7, 0.2, dw, db, N, H, W, 0.41) or True):
            chk(rz)
            ok('wgrad of the pool adjoint dw %+d' % pol, dw, rdw, TOL_WGRAD)
            ok('wgrad of the pool adjoint db %+d' % pol, db, rdb, TOL_WGRAD)
            ran = True
    return ran


@pytest.mark.parametrize('case', [(3, 32, 8, 8), (2, 64, 16, 8)])
def test_conv2d_unpooled_and_wgrad_unpooled(rz, case):
    N, H, cg, co = case
    assert unpooled_case(rz, N, H, H, cg, co)
    with tuning(3, 20), tuning(1, 20):                        # tile twins of the row-streaming kernels
        assert unpooled_case(rz, N, H, H, cg, co)


def test_y_bytes_and_mask_bytes(rz):
    N, H, ci, co = 3, 32, 8, 16
    G = rz.guard
    x, w, b = rnd(N, H, H, ci), rnd(3, 3, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    other = rnd(N, H // 2, H // 2, co, seed=3)
    xd, wd, bd, od = G(x), G(w), G(b), G(other)
    ry, ryp = E.conv2d_pool(x, w, b, N, H, H, 3, 1, 0.4, slope=0.2, other=other, a=0.6, b=0.4)
    yb, ypb = ops.conv2d_pool(xd, wd, bd, N, H, H, 3, 1, 0.4, 0.2, other=od, a=0.6, b=0.4, y_bytes=True)
    chk(rz)
    assert yb.dtype == torch.uint8 and float((yb.cpu() == E.signbytes_of(ry)).float().mean()) > 0.9999
    ok('y_bytes: pooled', ypb, ryp)
    m = rnd(N, H, H, co, seed=5)
    _, rt = E.conv2d_pool(x, w, None, N, H, H, 3, 1, 0.4, mask=m, mask_slope=0.2, other=other, a=0.6, b=0.4)
    g, wt = rnd(N, H // 2, H // 2, co, seed=4), rnd(3, 3, co, co, seed=5) * 0.2
    gd, wtd = G(g), G(wt)
    rup = E.conv2d_unpool(g, wt, N, H // 2, H // 2, 3, 1, 0.3, upmask=m, mul=0.7, mask_slope=0.2)
    for pol in POLARITIES:
        mb = G(E.signbytes_of(m), 'mask', pol)
        _, tb = ops.conv2d_pool(xd, wd, None, N, H, H, 3, 1, 0.4, 1.0, mask=mb, mask_slope=0.2, other=od, a=0.6, b=0.4, pool_only=True)
        chk(rz, may_stay_unwritten=POOL_ONLY_Y)
        ok('mask_bytes: masked conv + pool %+d' % pol, tb, rt)
        up = ops.conv2d_unpool(gd, wtd, N, H // 2, H // 2, 3, 1, 0.3, upmask=mb, mul=0.7, mask_slope=0.2)
        chk(rz, may_stay_unwritten=UNPOOL_SCRATCH_Y)
        ok('mask_bytes: unpool %+d' % pol, up, rup)
        ok('signbytes_to_mask %+d' % pol, ops.signbytes_to_mask(mb), E.signbytes_to_mask(E.signbytes_of(m)), 1e-7)
        chk(rz)


# ------------------------------------------------------------------- row-streaming kernels and their tile twins
@pytest.mark.parametrize('case', [(1, 64, 64, 8, 8), (9, 64, 64, 8, 8), (1, 64, 64, 16, 8)])
@pytest.mark.parametrize('twin', [False, True])
def test_row_streaming_conv_and_tile_twin(rz, case, twin):
    N, H, W, ci, co = case
    lib = pg._lib.load()
    if twin:
        assert lib.pg_debug_set_tuning(3, 20) == 0 and lib.pg_debug_set_tuning(1, 20) == 0
    names = []
    conv_case(rz, N, H, W, ci, co, 3, 1, 0)
    names.append(lib.pg_debug_last_conv_kernel().decode())      # the last launch of conv_case: the weight gradient
    pixelnorm_conv_case(rz, N, H, W, ci, co)
    names.append(lib.pg_debug_last_conv_kernel().decode())      # ... of pixelnorm_conv_case: the conv with the PixelNorm adjoint
    want = ('conv_wgrad_thin_kernel', 'conv_thin_kernel') if twin else ('wgrad_strip_kernel', 'conv_strip_kernel')
    assert [n.split('<')[0] for n in names] == list(want), names


def rgb_fused_case(rz, N, H, W, C):
    G = rz.guard
    img = rnd(N, C, H, W, seed=1)
    rw, rb = rnd(8, C, seed=2) * 0.7, rnd(8, seed=3) * 0.3
    w, b = rnd(3, 3, 8, 8, seed=4) * 0.2, rnd(8, seed=5) * 0.1
    # c1(fromRGB(img))
    ex0 = E.fromrgb_fwd(img, rw, rb, N, C, H, W, 0.61, 0.2)
    out = refused(rz, lambda: ops.conv2d_fromrgb(G(img, name='img'), G(rw), G(rb), 0.61, 0.2, G(w), G(b), N, C, H, W, 0.37, 0.2))
    if out is None:
        return False
    chk(rz)
    assert pg._lib.load().pg_debug_last_conv_kernel().decode().startswith('conv_strip_rgb_kernel')
    y, yb, xb = out
    ok('conv(fromRGB) y', y, E.conv2d(ex0, w, b, N, H, W, 3, 1, 0.37, slope=0.2))
    assert torch.equal(yb.cpu(), E.signbytes_of(y.cpu()))
    assert float((xb.cpu() == E.signbytes_of(ex0)).float().mean()) > 0.9999
    # conv + PixelNorm + toRGB
    x = rnd(N, H, W, 8, seed=1)
    tw, tb = rnd(C, 8, seed=4) * 0.5, rnd(C, seed=5) * 0.2
    y, r, im = ops.conv2d_pixelnorm_torgb(G(x), G(w), G(b), G(tw), G(tb), N, C, H, W, 0.37, 0.2, 0.71, 1e-8)
    chk(rz)
    ey, er = E.conv2d_pixelnorm(x, w, b, N, H, W, 3, 1, 0.37, 0.2, 1e-8)
    ok('conv+pn+toRGB y', y, ey)
    ok('conv+pn+toRGB r', r, er)
    ok('conv+pn+toRGB img', im, E.torgb_fwd(ey, tw, tb, N, C, H, W, 0.71))
    # masked backward conv + fromRGB's adjoint / weight gradient
    gz, wt, m = rnd(N, H, W, 8, seed=1), rnd(3, 3, 8, 8, seed=2) * 0.2, rnd(N, H, W, 8, seed=3)
    egf = E.conv2d(gz, wt, None, N, H, W, 3, 1, 0.37, mask=m, mask_slope=0.2)
    egi = torch.zeros(N, C, H, W)
    E.fromrgb_bwd_data(egf, rw, egi, N, C, H, W, 0.61)
    edw, edb = torch.full((8, C), 0.25), torch.full((8,), -0.5)
    E.fromrgb_wgrad(egf, img, edw, edb, N, C, H, W, 0.61)
    gzd, wtd, rwd, imgd = G(gz), G(wt), G(rw), G(img)
    for pol in POLARITIES:
        mb = G(E.signbytes_of(m), 'mask', pol)
        for keep, want_gimg in ((True, True), (False, True), (True, False), (False, False)):
            dw, db = G(torch.full((8, C, 1, 1), 0.25), 'acc', name='rgb_dw'), G(torch.full((8,), -0.5), 'acc', name='rgb_db')
            gf, gi = ops.conv2d_masked_fromrgb_bwd(gzd, wtd, mb, 0.2, rwd, 0.61, N, C, H, W, 0.37, keep_gf=keep, want_gimg=want_gimg,
                                                   img=imgd, rgb_dw=dw, rgb_db=db)
            chk(rz)
            assert (gf is None) == (not keep) and (gi is None) == (not want_gimg)
            if keep:
                ok('masked bwd conv gf', gf, egf)
            if want_gimg:
                ok('masked bwd conv gimg', gi, egi)
            ok('masked bwd conv rgb_dw', dw.view(8, C), edw, TOL_WGRAD)
            ok('masked bwd conv rgb_db', db, edb, TOL_WGRAD)
        gf, gi = ops.conv2d_masked_fromrgb_bwd(gzd, wtd, mb, 0.2, rwd, 0.61, N, C, H, W, 0.37)       # without the weight gradient
        chk(rz)
        ok('masked bwd conv gf (no wgrad)', gf, egf)
        ok('masked bwd conv gimg (no wgrad)', gi, egi)
    return True


@pytest.mark.parametrize('N,H,W,C', [(9, 32, 128, 1), (1, 16, 64, 2), (3, 64, 64, 3)])
def test_rgb_fused_row_streaming(rz, N, H, W, C):
    assert rgb_fused_case(rz, N, H, W, C)
    assert pg._lib.load().pg_debug_last_conv_kernel().decode().startswith('conv_strip_x_kernel<2, ')      # the masked backward conv ran last


# ----------------------------------------------------------------------------------------------------- Winograd
def wino_case(rz, N, H, W, ci, co, ups, epilogues=True):
    G = rz.guard
    hin, win = (H // 2, W // 2) if ups else (H, W)
    x, w, b = rnd(N, hin, win, ci), rnd(3, 3, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    m, other, um = rnd(N, H, W, co, seed=3), rnd(N, H // 2, W // 2, co, seed=4), rnd(N, 2 * H, 2 * W, co, seed=5)
    xd, bd = G(x), G(b)
    u = refused(rz, lambda: ops.wino_transform_weights(G(w)))
    if u is None:
        return False
    chk(rz)
    ok('weight transform', ops.wino_unpack(u), E.wino_transform_weights(w), 1e-6)
    ref = E.conv2d(x, w, b, N, H, W, 3, 1, 0.37, slope=0.2, ups=bool(ups))
    refm = E.conv2d(x, w, None, N, H, W, 3, 1, 0.37, mask=m, mask_slope=0.2, ups=bool(ups))
    y = refused(rz, lambda: ops.conv2d_wino(xd, u, bd, N, H, W, 0.37, 0.2, ups=bool(ups)))
    if y is None:
        return False
    chk(rz)
    ok('wino fwd', y, ref)
    for pol in POLARITIES:
        y = ops.conv2d_wino(xd, u, None, N, H, W, 0.37, mask=G(m, 'mask', pol), mask_slope=0.2, ups=bool(ups))
        chk(rz)
        ok('wino masked fp32 %+d' % pol, y, refm)
        if not ups:
            y = ops.conv2d_wino(xd, u, None, N, H, W, 0.37, mask=G(E.signbytes_of(m), 'mask', pol), mask_slope=0.2)
            chk(rz)
            ok('wino masked bytes %+d' % pol, y, refm)
    if ups or not epilogues:
        return True
    od = G(other)
    y, yp = ops.conv2d_wino(xd, u, bd, N, H, W, 0.37, 0.2, pool=True, other=od, a=0.6, b=0.4)
    chk(rz)
    ry, ryp = E.conv2d_pool(x, w, b, N, H, W, 3, 1, 0.37, slope=0.2, other=other, a=0.6, b=0.4)
    ok('wino+pool y', y, ry)
    ok('wino+pool ypool', yp, ryp)
    _, yp = ops.conv2d_wino(xd, u, None, N, H, W, 0.37, pool=True, a=4.0, pool_only=True)
    chk(rz, may_stay_unwritten=POOL_ONLY_Y)
    ok('wino pool only', yp, E.conv2d_pool(x, w, None, N, H, W, 3, 1, 0.37, a=4.0)[1])
    rup = E.conv2d_unpool(x, w, N, H, W, 3, 1, 0.37, upmask=um, mul=0.7, mask_slope=0.2)
    for pol in POLARITIES:
        for umd in (G(um, 'mask', pol), G(E.signbytes_of(um), 'mask', pol)):
            yu = ops.conv2d_wino(xd, u, None, N, H, W, 0.37, mask_slope=0.2, unpool=True, upmask=umd, up_mul=0.7)
            # the wrapper allocates a full-resolution y for every form but returns only yup here: y is not a returned output
            chk(rz, may_stay_unwritten=[r.view for r in rz.records if r.role == 'out' and r.view.data_ptr() != yu.data_ptr()])
            ok('wino+unpool %+d %s' % (pol, umd.dtype), yu, rup)
    yb, yp = ops.conv2d_wino(xd, u, bd, N, H, W, 0.37, 0.2, pool=True, y_bytes=True)
    chk(rz)
    ry, ryp = E.conv2d_pool(x, w, b, N, H, W, 3, 1, 0.37, slope=0.2)
    ok('wino y_bytes: pooled', yp, ryp)
    assert float((yb.cpu() == E.signbytes_of(ry)).float().mean()) > 0.9999
    y, ys = ops.conv2d_wino(xd, u, bd, N, H, W, 0.37, 0.2, signs_out=True)
    chk(rz)
    ok('wino signs_out y', y, ref)
    assert bool((ys.cpu() == E.signbytes_of(y.cpu())).all())
    return True


WINO_CASES = [(3, 16, 128, 96, 0), (1, 8, 32, 48, 0), (3, 8, 64, 36, 0), (2, 32, 64, 48, 1), (1, 32, 36, 48, 0)]


@pytest.mark.parametrize('case', WINO_CASES)
@pytest.mark.parametrize('variant,ksplit', [(0, -1), (11, -1), (12, -1), (20, -1), (21, -1), (0, 2), (0, 3)])
def test_conv2d_wino(rz, case, variant, ksplit):
    N, H, ci, co, ups = case
    lib = pg._lib.load()
    assert lib.pg_debug_set_wino(variant) == 0 and lib.pg_debug_set_wino_ksplit(ksplit) == 0
    if ci % 8:
        with pytest.raises(RuntimeError):                     # "Cin % 8 == 0": PG_E_ALIGN before anything is launched (this case is for the weight gradient)
            ops.conv2d_wino(rz.guard(rnd(N, H, H, ci)), rz.guard(rnd(16, co, ci)), None, N, H, H, 0.37, 0.2)
        rz.discard_outputs()
        return
    assert wino_case(rz, N, H, H, ci, co, ups, epilogues=(variant in (0, 21) or ksplit > 0))


@pytest.mark.parametrize('case', [(1, 128, 8, 32, 0), (1, 128, 16, 32, 1)])
def test_conv2d_wino_row_streaming(rz, case):
    N, H, ci, co, ups = case
    lib = pg._lib.load()
    assert lib.pg_debug_set_wino(21) == 0
    assert wino_case(rz, N, H, H, ci, co, ups)
    assert lib.pg_debug_last_wino_kernel().decode().startswith('conv_wino_strip_kernel<%d, ' % ci)


def wino_pn_case(rz, N, H, W, ci, co, ups):
    G = rz.guard
    hin, win = (H // 2, W // 2) if ups else (H, W)
    x, w, b = rnd(N, hin, win, ci), rnd(3, 3, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    u = ops.wino_transform_weights(G(w))
    chk(rz)
    if co > 32:
        with pytest.raises(ops.Unsupported):                  # "Cout <= 32 (PG_E_UNSUP otherwise; wider layers normalise in a second pass)"
            ops.conv2d_wino_pixelnorm(G(x), u, G(b), N, H, W, 0.37, 0.2, 1e-8, ups=bool(ups))
        rz.discard_outputs()
        return
    out = refused(rz, lambda: ops.conv2d_wino_pixelnorm(G(x), u, G(b), N, H, W, 0.37, 0.2, 1e-8, ups=bool(ups)))
    if out is None:
        return False
    chk(rz)
    ry, rr = E.conv2d_pixelnorm(x, w, b, N, H, W, 3, 1, 0.37, 0.2, 1e-8, ups=bool(ups))
    ok('wino+pixelnorm y', out[0], ry)
    ok('wino+pixelnorm r', out[1], rr.reshape(-1))
    if ups:
        return True
    xd = G(x)
    for pool in (False, True):
        ho, wo = (H // 2, W // 2) if pool else (H, W)
        ys, rs, other = rnd(N, ho, wo, co, seed=2), rnd(N * ho * wo, seed=3).abs() + 0.5, rnd(N, ho, wo, co, seed=4)
        for oth in ((None, other) if pool else (None,)):
            ref = E.conv2d_wino_pnbwd(x, E.wino_transform_weights(w), ys, rs, N, H, W, 0.37, 0.2, pool=pool, other=oth, a=4.0,
                                      b=1.0 if oth is not None else 0.0)
            for kind, pol in (('data', 1), ('mask', 1), ('mask', -1)):
                y = ops.conv2d_wino_pnbwd(xd, u, G(ys, kind, pol), G(rs), N, H, W, 0.37, 0.2, pool=pool, other=G(oth), a=4.0,
                                          b=1.0 if oth is not None else 0.0)
                chk(rz)
                ok('wino+pnbwd pool=%s %s%+d' % (pool, kind, pol), y, ref, 3e-5)          # (test_winograd.py's bound for this entry point)
    return True


@pytest.mark.parametrize('case', [(1, 8, 32, 48, 0), (2, 32, 64, 24, 1), (3, 8, 64, 32, 0), (1, 32, 16, 8, 0)])
def test_conv2d_wino_pixelnorm_and_pnbwd(rz, case):
    N, H, ci, co, ups = case
    assert wino_pn_case(rz, N, H, H, ci, co, ups) is not False


def wino_wgrad_case(rz, N, H, W, ci, co, ups):
    G = rz.guard
    hin, win = (H // 2, W // 2) if ups else (H, W)
    x, gz = rnd(N, hin, win, ci), rnd(N, H, W, co, seed=1)
    dw0, db0 = rnd(3, 3, co, ci, seed=2), rnd(co, seed=3)
    rdw, rdb = dw0.clone(), db0.clone()
    E.conv2d_wgrad(x, gz, rdw, rdb, N, H, W, 3, 1, 0.41, ups=bool(ups))
    xd, gzd = G(x), G(gz)
    for with_db in (True, False):
        dw, db = G(dw0, 'acc'), G(db0, 'acc') if with_db else None
        if refused(rz, lambda: ops.conv2d_wgrad_wino(xd, gzd, dw, db, N, H, W, 0.41, ups=bool(ups)) or True) is None:
            return False
        chk(rz)
        ok('wino wgrad dw db=%s' % with_db, dw, rdw, TOL)
        if with_db:
            ok('wino wgrad db', db, rdb, TOL)
    # two batches of the same layer in one launch
    x2, gz2 = rnd(N + 1, hin, win, ci, seed=4), rnd(N + 1, H, W, co, seed=5)
    for bias2 in (False, True):
        rdw, rdb = dw0.clone(), db0.clone()
        E.conv2d_wgrad_wino(x, gz, rdw, rdb, N, H, W, 0.41, ups=bool(ups), second=(x2, gz2, N + 1, bias2))
        dw, db = G(dw0, 'acc'), G(db0, 'acc')
        ops.conv2d_wgrad_wino(xd, gzd, dw, db, N, H, W, 0.41, ups=bool(ups), second=(G(x2), G(gz2), N + 1, bias2))
        chk(rz)
        ok('wino wgrad two batches dw bias2=%s' % bias2, dw, rdw, TOL)
        ok('wino wgrad two batches db bias2=%s' % bias2, db, rdb, TOL)
    return True


@pytest.mark.parametrize('case', [(3, 16, 128, 96, 0), (1, 8, 32, 48, 0), (3, 8, 64, 36, 0), (2, 32, 64, 48, 1), (1, 32, 36, 48, 0),
                                  (4, 32, 256, 256, 0)])          # (the last: >= 6 regions per workgroup, the wave-pair mapping)
def test_conv2d_wgrad_wino(rz, case):
    N, H, ci, co, ups = case
    if H < 8 or H < 16:                                        # "H, W powers of two with H >= 8, W >= 16": refused below
        with pytest.raises(ops.Unsupported):
            ops.conv2d_wgrad_wino(rz.guard(rnd(N, H, H, ci)), rz.guard(rnd(N, H, H, co)), rz.guard(rnd(3, 3, co, ci), 'acc'), None, N, H, H, 0.41)
        return
    assert wino_wgrad_case(rz, N, H, H, ci, co, ups)
    if ci == 256:
        assert pg._lib.load().pg_debug_last_wino_wgrad_kernel().decode() == 'conv_wino_wgrad_pair_kernel'


def test_weight_transforms_batched_in_flat_buffers(rz):
    """Layers back to back at 16-byte granularity in guarded FLAT buffers (network.py / optim.py round every view to 4 floats and no
    more): a layer that overruns its slot corrupts its neighbour's payload, so every layer is compared."""
    G = rz.guard
    shapes = [(36, 8), (12, 24), (96, 128), (20, 40)]           # (cout, cin): cin % 8 == 0, couts that are no multiple of 16
    ws = [rnd(3, 3, co, ci, seed=7 + i) * 0.3 for i, (co, ci) in enumerate(shapes)]
    offs, uoffs, o, uo = [], [], 0, 0
    for (co, ci) in shapes:
        offs.append(o); uoffs.append(uo)
        o += 9 * co * ci; uo += 16 * co * ci
        assert o % 4 == 0 and uo % 4 == 0
    flat = G(torch.cat([w.reshape(-1) for w in ws]), name='flat w')
    # forward forms
    fu = rz.out((uo,), name='flat u')
    ops.wino_transform_weights_batched(flat, fu, [(offs[i], uoffs[i], co, ci) for i, (co, ci) in enumerate(shapes)])
    chk(rz)
    for i, (co, ci) in enumerate(shapes):
        ok('batched transform layer %d' % i, ops.wino_unpack(fu[uoffs[i]:uoffs[i] + 16 * co * ci].view(16, co, ci)), E.wino_transform_weights(ws[i]), 1e-6)
    # backward-data forms straight from the forward parameter (cin' = co must be a multiple of 8: the layers that qualify)
    tshapes = [(co, ci) for (co, ci) in shapes if co % 8 == 0]
    tl = [(offs[shapes.index(s)], uoffs[shapes.index(s)], s[1], s[0]) for s in tshapes]
    fu = rz.out((uo,), name='flat u (transposed)', fill=0.0)
    ops.wino_transform_weights_batched(flat, fu, tl, transposed=True)
    chk(rz)
    host = torch.zeros(uo)
    E.wino_transform_weights_batched(flat.cpu(), host, tl, transposed=True)
    for (woff, uoff, co_, ci_) in tl:
        ok('batched transposed transform', ops.wino_unpack(fu[uoff:uoff + 16 * co_ * ci_].view(16, co_, ci_)), host[uoff:uoff + 16 * co_ * ci_].view(16, co_, ci_), 1e-6)
    # pg_pack_dgrad_weights and its batched form over mixed kernel sizes
    pshapes = [(3, 20, 12), (1, 16, 8), (4, 32, 16), (3, 36, 8)]
    pws = [rnd(ks, ks, co, ci, seed=3 + i) for i, (ks, co, ci) in enumerate(pshapes)]
    poffs, o = [], 0
    for pw in pws:
        poffs.append(o); o += pw.numel()
    pflat = G(torch.cat([pw.reshape(-1) for pw in pws]), name='flat w (pack)')
    mirror = rz.out((o,), name='flat wt')
    ops.pack_dgrad_weights_batched(pflat, mirror, [(poffs[i], ks, co, ci) for i, (ks, co, ci) in enumerate(pshapes)])
    chk(rz)
    for i, (ks, co, ci) in enumerate(pshapes):
        ref = torch.empty(ks, ks, ci, co)
        E.pack_dgrad_weights(pws[i], ref)
        assert torch.equal(mirror[poffs[i]:poffs[i] + pws[i].numel()].view(ks, ks, ci, co).cpu(), ref)
        wt = rz.out((ks, ks, ci, co))
        ops.pack_dgrad_weights(G(pws[i]), wt)
        chk(rz)
        assert torch.equal(wt.cpu(), ref)


# ----------------------------------------------------------------------------------------------------- rgb.hip
def rgb_case(rz, N, C, H, W, co):
    G = rz.guard
    for pool in (False, True):
        hi, wi = (2 * H, 2 * W) if pool else (H, W)
        img, w, b = rnd(N, C, hi, wi), rnd(co, C, seed=1), rnd(co, seed=2)
        imgd, wd = G(img, name='img'), G(w, name='rgb w')
        y = ops.fromrgb_fwd(imgd, wd, G(b), N, C, H, W, 0.8, 0.2, pool=pool)
        chk(rz)
        ok('fromrgb fwd pool=%s' % pool, y, E.fromrgb_fwd(img, w, b, N, C, H, W, 0.8, 0.2, pool=pool))
        out = refused(rz, lambda: ops.fromrgb_fwd(imgd, wd, G(b), N, C, H, W, 0.8, 0.2, pool=pool, signs_out=True))
        if out is not None:
            chk(rz)
            assert torch.equal(out[1].cpu(), E.signbytes_of(out[0].cpu()))
        m = rnd(N, H, W, co, seed=3)
        rm = E.fromrgb_fwd(img, w, None, N, C, H, W, 0.8, 1.0, pool=pool, mask=m, mask_slope=0.2)
        for pol in POLARITIES:
            for md in (G(m, 'mask', pol), G(E.signbytes_of(m), 'mask', pol)):
                y = refused(rz, lambda: ops.fromrgb_fwd(imgd, wd, None, N, C, H, W, 0.8, 1.0, pool=pool, mask=md, mask_slope=0.2))
                if y is not None:
                    chk(rz)
                    ok('fromrgb masked %+d %s' % (pol, md.dtype), y, rm)
        gz = rnd(N, H, W, co, seed=4)
        gzd = G(gz)
        g0 = rnd(N, C, hi, wi, seed=5)
        for acc in (False, True):
            gi = G(g0, 'acc', name='gimg') if acc else rz.out((N, C, hi, wi), name='gimg')
            ops.fromrgb_bwd_data(gzd, wd, gi, N, C, H, W, 0.8, pool=pool, accumulate=acc)
            chk(rz)
            r = g0.clone()
            E.fromrgb_bwd_data(gz, w, r, N, C, H, W, 0.8, pool=pool, accumulate=acc)
            ok('fromrgb bwd_data acc=%s' % acc, gi, r)
        dw0, db0 = rnd(co, C, seed=6), rnd(co, seed=7)
        dw, db = G(dw0, 'acc', name='rgb dw'), G(db0, 'acc', name='rgb db')
        ops.fromrgb_wgrad(gzd, imgd, dw, db, N, C, H, W, 0.8, pool=pool)
        chk(rz)
        rw, rb = dw0.clone(), db0.clone()
        E.fromrgb_wgrad(gz, img, rw, rb, N, C, H, W, 0.8, pool=pool)
        ok('fromrgb wgrad', dw, rw, TOL_WGRAD)
        ok('fromrgb bgrad', db, rb, TOL_WGRAD)
    ci = co
    x, w, b = rnd(N, H, W, ci), rnd(C, ci, seed=1), rnd(C, seed=2)
    prev = rnd(N, C, H // 2, W // 2, seed=3)
    xd, wd, bd = G(x), G(w, name='torgb w'), G(b, name='torgb bias')
    y = ops.torgb_fwd(xd, wd, bd, N, C, H, W, 0.7)
    chk(rz)
    ok('torgb fwd', y, E.torgb_fwd(x, w, b, N, C, H, W, 0.7))
    if H % 2 == 0 and W % 2 == 0:
        y = ops.torgb_fwd(xd, wd, bd, N, C, H, W, 0.7, out_mul=0.3, prev=G(prev), prev_mul=0.7)
        chk(rz)
        ok('torgb blend', y, E.torgb_fwd(x, w, b, N, C, H, W, 0.7, out_mul=0.3, prev=prev, prev_mul=0.7))
    g, g2 = rnd(N, C, H, W, seed=4), rnd(N, C, 2 * H, 2 * W, seed=5)
    gd, g2d = G(g), G(g2)
    gx = ops.torgb_bwd_data(gd, wd, N, C, H, W, 0.21)
    chk(rz)
    ok('torgb bwd_data', gx, E.torgb_bwd_data(g, w, N, C, H, W, 0.21))
    gx = ops.torgb_bwd_data(g2d, wd, N, C, H, W, 0.21, down=True)
    chk(rz)
    ok('torgb bwd_data down', gx, E.torgb_bwd_data(g2, w, N, C, H, W, 0.21, down=True))
    ys, rs = rnd(N, H, W, ci, seed=8), rnd(N * H * W, seed=9).abs() + 0.5
    ref = E.torgb_bwd_data_pnbwd(g, w, ys, rs, N, C, H, W, 0.21, 0.2)
    for kind, pol in (('data', 1), ('mask', 1), ('mask', -1)):
        gx = ops.torgb_bwd_data_pnbwd(gd, wd, G(ys, kind, pol), G(rs), N, C, H, W, 0.21, 0.2)
        # where the fused kernel does not exist the wrapper returns the buffer of its two-launch fallback and drops the one it
        # allocated first: that one is not a returned output (it never reached a kernel)
        dropped = [r.view for r in rz.records if r.name == 'torgb_bwd_data_pnbwd:0' and r.view.data_ptr() != gx.data_ptr()]
        chk(rz, may_stay_unwritten=dropped)
        ok('torgb bwd_data + pn adjoint %s%+d' % (kind, pol), gx, ref)
    for down, gg, ggd in ((False, g, gd), (True, g2, g2d)):
        dw0, db0 = rnd(C, ci, seed=6), rnd(C, seed=7)
        dw, db = G(dw0, 'acc', name='torgb dw'), G(db0, 'acc', name='torgb db')
        ops.torgb_wgrad(ggd, xd, dw, db, N, C, H, W, 0.21, 0.3, down=down)
        chk(rz)
        rw, rb = dw0.clone(), db0.clone()
        E.torgb_wgrad(gg, x, rw, rb, N, C, H, W, 0.21, 0.3, down=down)
        ok('torgb wgrad down=%s' % down, dw, rw, TOL_WGRAD)
        ok('torgb bgrad down=%s' % down, db, rb, TOL_WGRAD)


@pytest.mark.parametrize('N,C,H,co', [(3, 1, 8, 32), (2, 4, 8, 12), (2, 3, 4, 512), (1, 3, 256, 8)])
def test_rgb_layers(rz, N, C, H, co):
    rgb_case(rz, N, C, H, H, co)


# ------------------------------------------------------------------------------------------------ elementwise.hip
def pool_up_case(rz, N, H, W, C):
    G = rz.guard
    x, o = rnd(N, 2 * H, 2 * W, C), rnd(N, H, W, C, seed=1)
    xd = G(x)
    y = ops.avgpool2_fwd(xd); chk(rz)
    ok('avgpool', y, E.avgpool2_fwd(x))
    y = ops.avgpool2_fwd(xd, G(o), 0.3, 0.7); chk(rz)
    ok('avgpool blend', y, E.avgpool2_fwd(x, o, 0.3, 0.7))
    gy, m = rnd(N, H, W, C, seed=2), rnd(N, 2 * H, 2 * W, C, seed=3)
    gyd = G(gy)
    y = ops.avgpool2_bwd(gyd); chk(rz)
    ok('avgpool bwd nomask', y, E.avgpool2_bwd(gy))
    y = ops.upsample2_bwd(xd); chk(rz)
    ok('upsample bwd', y, E.upsample2_bwd(x))
    y = ops.axpby_mask(xd, a=0.3); chk(rz)
    ok('scale', y, E.axpby_mask(x, a=0.3))
    for pol in POLARITIES:
        md = G(m, 'mask', pol)
        y = ops.avgpool2_bwd(gyd, md, 0.3, 0.2); chk(rz)
        ok('avgpool bwd %+d' % pol, y, E.avgpool2_bwd(gy, m, 0.3, 0.2))
        y = ops.axpby_mask(xd, G(m), md, 0.3, 0.7, 0.2); chk(rz)
        ok('axpby %+d' % pol, y, E.axpby_mask(x, m, m, 0.3, 0.7, 0.2))


@pytest.mark.parametrize('N,H,C', [(2, 2, 4), (3, 4, 512)])
def test_pool_upsample_axpby(rz, N, H, C):
    pool_up_case(rz, N, H, H, C)


@pytest.mark.parametrize('P,C', [(37, 4), (5, 32), (300, 256)])
def test_pixelnorm(rz, P, C):
    G = rz.guard
    x, gy, t, a = rnd(P, C), rnd(P, C, seed=1), rnd(P, C, seed=2), rnd(P, C, seed=3)
    ry, rr = E.pixelnorm_fwd(x)
    y, r = ops.pixelnorm_fwd(G(x)); chk(rz)
    ok('pn fwd', y, ry)
    ok('pn r', r, rr)
    xi = G(x, inplace=True)
    y, r = ops.pixelnorm_fwd(xi, inplace=True); chk(rz)
    ok('pn fwd in place', xi, ry)
    gyd, rd = G(gy), G(rr)
    ty, inj = ops.pixelnorm_tangent(G(t), G(ry), rd, G(a)); chk(rz)
    rty, rinj = E.pixelnorm_tangent(t, ry, rr, a)
    ok('pn tangent', ty, rty, TOL_HVP)
    ok('pn injection', inj, rinj, TOL_HVP)
    for kind, pol in (('data', 1), ('mask', 1), ('mask', -1)):
        yd = G(ry, kind, pol)
        gz = ops.pixelnorm_lrelu_bwd(gyd, yd, rd, 0.2); chk(rz)
        ok('pn bwd %s%+d' % (kind, pol), gz, E.pixelnorm_lrelu_bwd(gy, ry, rr, 0.2))
        gz = ops.pixelnorm_lrelu_bwd(gyd, yd, None, 0.2); chk(rz)
        ok('lrelu-only bwd %s%+d' % (kind, pol), gz, E.pixelnorm_lrelu_bwd(gy, ry, None, 0.2))
        gz = ops.pixelnorm_lrelu_bwd(gyd, yd, rd, 0.2, inj=G(rinj)); chk(rz)
        ok('pn bwd + injection %s%+d' % (kind, pol), gz, E.pixelnorm_lrelu_bwd(gy, ry, rr, 0.2, inj=rinj), TOL_HVP)
    gi = G(gy, inplace=True)
    ops.pixelnorm_lrelu_bwd(gi, G(ry, 'mask', -1), rd, 0.2, inplace=True); chk(rz)
    ok('pn bwd in place', gi, E.pixelnorm_lrelu_bwd(gy.clone(), ry, rr, 0.2))


@pytest.mark.parametrize('G_,n,C', [(2, 5, 32), (3, 3, 512)])
def test_mbstd_local_and_exact_global(rz, G_, n, C):
    G = rz.guard
    cp = C + 16
    x = rnd(G_ * n, 4, 4, C) + 0.3
    tx = rnd(G_ * n, 4, 4, C, seed=1)
    gy, gf = rnd(G_ * n, 4, 4, cp, seed=2), rnd(G_ * n, 4, 4, cp, seed=3)
    ry, rst = E.mbstd_fwd(x, G_, cp)
    rty, rts = E.mbstd_tangent(x, tx, rst, cp)
    txd, gyd, gfd = G(tx), G(gy), G(gf)
    xd = G(x)
    y, st = ops.mbstd_fwd(xd, G_, cp); chk(rz, may_stay_unwritten=MBSTD_STATS)
    ok('mbstd fwd', y, ry)
    ok('mbstd stats', st[:, :2], rst)
    ty, ts = ops.mbstd_tangent(xd, txd, st, cp); chk(rz, may_stay_unwritten=MBSTD_STATS)
    ok('mbstd tangent', ty, rty)
    ok('mbstd tstats', ts[:, :2], rts, TOL_HVP)
    for am in (False, True):
        for kind, pol in ((('data', 1), ('mask', 1), ('mask', -1)) if am else (('data', 1),)):      # x enters through x > 0 when the mask is applied
            xk = G(x, kind, pol)
            gx = ops.mbstd_bwd(gyd, xk, st, cp, am, 0.2); chk(rz)
            ok('mbstd bwd mask=%s %s%+d' % (am, kind, pol), gx, E.mbstd_bwd(gy, x, rst, cp, am, 0.2))
            gx = ops.mbstd_bwd(gyd, xk, st, cp, am, 0.2, tx=txd, tstats=ts, gy_first=gfd); chk(rz)
            ok('mbstd bwd+hvp', gx, E.mbstd_bwd(gy, x, rst, cp, am, 0.2, tx=tx, tstats=rts, gy_first=gf), TOL_HVP)
            gx = ops.mbstd_bwd(None, xk, st, cp, am, 0.2, tx=txd, tstats=ts, gy_first=gfd); chk(rz)
            ok('mbstd hvp only', gx, E.mbstd_bwd(None, x, rst, cp, am, 0.2, tx=tx, tstats=rts, gy_first=gf), TOL_HVP)
    # exact-global entry points with one "rank" (gathered = this rank's partial row)
    part = ops.mbstd_stats(xd, G_); chk(rz, may_stay_unwritten=MBSTD_STATS)
    gathered = G(part.clone().unsqueeze(0).contiguous())
    stg = G(part.clone(), inplace=True)
    y, stg = ops.mbstd_write(xd, stg, gathered, cp); chk(rz)
    ok('global mbstd fwd', y, ry)
    ok('global mbstd stats', stg[:, :2], rst)
    tpart = ops.mbstd_tangent_stats(xd, txd, stg); chk(rz, may_stay_unwritten=MBSTD_STATS)
    tg = G(tpart.clone().unsqueeze(0).contiguous())
    tsg = G(tpart.clone(), inplace=True)
    ty, tsg = ops.mbstd_tangent_write(txd, tsg, tg, stg, cp); chk(rz)
    ok('global mbstd tangent', ty, rty, TOL_HVP)
    ok('global mbstd tstats', tsg[:, :2], rts, TOL_HVP)
    gsum = ops.mbstd_gsum(gyd, gfd, G_, tuple(x.shape), cp); chk(rz)
    ok('global mbstd gsum', gsum, torch.stack([torch.stack([gy[g * n:(g + 1) * n][..., C].double().sum(), gf[g * n:(g + 1) * n][..., C].double().sum()])
                                                for g in range(G_)]), TOL)
    got = ops.mbstd_bwd_global(gyd, xd, stg, cp, True, gsum, 1, 0.2, tx=txd, tstats=tsg, gy_first=gfd); chk(rz)
    ok('global mbstd bwd', got, E.mbstd_bwd(gy, x, rst, cp, True, 0.2, tx=tx, tstats=rts, gy_first=gf), TOL_HVP)


@pytest.mark.parametrize('N,C', [(9, 512), (1, 512)])
def test_linear_gp_loss(rz, N, C):
    G = rz.guard
    h, w, b = rnd(N, 1, 1, C), rnd(1, C, seed=1), rnd(1, seed=2)
    hd, wd = G(h), G(w)
    s = ops.linear1_fwd(hd, wd, G(b)); chk(rz)
    ok('linear fwd', s, E.linear1_fwd(h, w, b))
    gs = rnd(N, seed=3)
    gsd = G(gs)
    for pol in POLARITIES:
        gh = ops.linear1_bwd_data(gsd, wd, G(h, 'mask', pol), h.shape, 0.2); chk(rz)
        ok('linear bwd %+d' % pol, gh, E.linear1_bwd_data(gs, w, h, h.shape, 0.2))
    dw0, db0 = rnd(1, C, seed=4), rnd(1, seed=5)
    dw, db = G(dw0, 'acc'), G(db0, 'acc')
    ops.linear1_wgrad(gsd, hd, dw, db); chk(rz)
    rw, rb = dw0.clone(), db0.clone()
    E.linear1_wgrad(gs, h, rw, rb)
    ok('linear wgrad', dw, rw)
    ok('linear bgrad', db, rb)
    real, fake, m = rnd(N, 3, 16, 16), rnd(N, 3, 16, 16, seed=1), torch.rand(N, generator=torch.Generator().manual_seed(5))
    reald = G(real)
    mixed = ops.gp_mix(reald, G(fake), G(m)); chk(rz)
    ok('gp mix', mixed, E.gp_mix(real, fake, m))
    ss = ops.row_sumsq(reald); chk(rz)
    ok('row sumsq', ss, E.row_sumsq(real))
    gp, u = ops.gp_seed(reald, G(E.row_sumsq(real)), 10.0, 1.0, 0.25); chk(rz)
    rgp, ru = E.gp_seed(real, E.row_sumsq(real), 10.0, 1.0, 0.25)
    ok('gp', gp, rgp)
    ok('gp seed', u, ru)
    sc, gpv = rnd(3 * N, seed=7), torch.rand(N, generator=torch.Generator().manual_seed(6))
    scd = G(sc)
    out = ops.d_loss(scd, G(gpv), N, 0.001); chk(rz)
    for nm, a, r in zip(('d_cost', 'd_real_loss', 'd_fake_loss', 'gscore'), out, E.d_loss(sc, gpv, N, 0.001)):
        ok('d_loss ' + nm, a, r)
    gc, gsc = ops.g_loss(scd); chk(rz)
    rgc, rgsc = E.g_loss(sc)
    ok('g_cost', gc, rgc)
    ok('g gscore', gsc, rgsc)


@pytest.mark.parametrize('n', [1003, 4, 4100])
def test_adam_ema_zero(rz, n):
    G = rz.guard
    npad = n + (-n % 4)                                        # flat-buffer segments are rounded to 4 floats (network.py, optim.py)
    p, g, mm, vv = rnd(npad), rnd(npad, seed=1), rnd(npad, seed=2) * 0.1, rnd(npad, seed=3).abs() * 0.1
    dp, dg, dm, dv = G(p, 'acc', name='adam p'), G(g, name='adam g'), G(mm, 'acc', name='adam m'), G(vv, 'acc', name='adam v')
    for args in ((1e-3, 0.0, 0.99, 1e-8, 1.0, 0.3, 0.5), (2e-3, 0.9, 0.999, 1e-8, 0.19, 0.0447, 1.0)):
        ops.adam(dp, dg, dm, dv, *args); chk(rz)
        E.adam(p, g, mm, vv, *args)
        ok('adam p', dp, p)
        ok('adam m', dm, mm)
        ok('adam v', dv, vv)
    avg, q = rnd(npad, seed=4), rnd(npad, seed=5)
    da = G(avg, 'acc', name='ema avg')
    ops.ema(da, G(q, name='ema p'), 0.999); chk(rz)
    want = torch.addcmul(avg, torch.tensor(1 - 0.999, dtype=torch.float32), q - avg)
    ok('ema', da, want, 1e-6)
    z = G(rnd(npad), inplace=True, name='zeroed')
    ops.zero_(z); chk(rz)
    assert not bool(z.any())


@pytest.mark.parametrize('n', [3, 4099])
def test_uniform(rz, n):
    seed, offset = (5 << 40) + 3, (9 << 33) + 1
    out = rz.out((n,))
    ops.uniform_(out, seed, offset); chk(rz)
    got = out.cpu().numpy()
    for i in sorted(set(list(range(min(n, 12))) + [n - 1, n // 2])):
        w = _philox4x32_10([(i // 4) & 0xffffffff, (i // 4) >> 32, offset & 0xffffffff, offset >> 32], [seed & 0xffffffff, seed >> 32])[i % 4]
        assert float(got[i]) == (w >> 8) / 16777216.0, (i, got[i])
    assert got.min() >= 0.0 and got.max() < 1.0


# ------------------------------------------------------------------------------------------------------ workspace
@pytest.mark.parametrize('kind,N,H,ci,co', [(0, 3, 16, 256, 256), (1, 9, 4, 80, 32)])
def test_workspace_launch_stays_inside_the_queried_size(rz, kind, N, H, ci, co):
    """pg_workspace_bytes: a scratch of EXACTLY the queried size, 16-byte aligned ("caller owns `ptr` (16-byte aligned, ZERO-FILLED
    once ...)"), inside a guarded zero-filled buffer, registered for a side stream.  The K-sliced launch must stay inside it.  The
    header promises "self-resetting tickets", not that the partial sums are cleared, so only the bands and the result are asserted."""
    lib = pg._lib.load()
    need = ops.workspace_bytes(kind, N, H, H, ci, co)
    assert need > 0 and need % 16 == 0
    scratch = rz.out((need,), torch.uint8, name='scratch', fill=0)
    ks = 3 if kind == 0 else 4
    x, w, b = rnd(N, H, H, ci), rnd(ks, ks, co, ci, seed=1) * 0.2, rnd(co, seed=2)
    xd, wd, bd = rz.guard(x), rz.guard(w), rz.guard(b)
    if kind == 0:
        ud = ops.wino_transform_weights(wd)
        run = lambda: ops.conv2d_wino(xd, ud, bd, N, H, H, 0.37, 0.2)
        last = lib.pg_debug_last_wino_kernel
    else:
        run = lambda: ops.conv2d(xd, wd, bd, N, H, H, 4, 0, 0.37, slope=0.2)
        last = lib.pg_debug_last_conv_kernel
    side = torch.cuda.Stream()
    h = ctypes.c_void_p(side.cuda_stream)
    torch.cuda.synchronize()
    assert lib.pg_set_workspace(h, ctypes.c_void_p(scratch.data_ptr()), need) == 0
    try:
        ops._workspaces[(torch.cuda.current_device(), side.cuda_stream)] = None       # ops must not register its own for this stream
        with torch.cuda.stream(side):
            ys = [run() for _ in range(2)]                      # twice: the tickets reset themselves
            name = last().decode()
        side.synchronize()
        chk(rz, keep_outputs=True)
        assert (', true, ' in name) if kind == 0 else name.startswith('conv_k4_reduce_split_kernel'), name
    finally:
        side.synchronize()
        assert lib.pg_set_workspace(h, None, 0) == 0
        ops._workspaces.pop((torch.cuda.current_device(), side.cuda_stream), None)
    if kind == 0:
        lib.pg_debug_set_wino_ksplit(0)
    else:
        lib.pg_debug_set_tuning(3, 21)
    unsplit = run()
    chk(rz)
    ref = E.conv2d(x, w, b, N, H, H, ks, 3 - ks + 1 if kind == 0 else 0, 0.37, slope=0.2)
    assert torch.equal(ys[0], ys[1])
    ok('sliced vs unsplit', ys[0], unsplit, 1e-6)
    ok('sliced vs contract', ys[0], ref)


# ------------------------------------------------------------------------------------------------ non-square maps
NONSQUARE = [(3, 8, 16), (3, 16, 8)]
NONSQUARE_STRIP = [(1, 64, 128), (1, 128, 64)]


@pytest.mark.parametrize('N,H,W', NONSQUARE)
@pytest.mark.parametrize('ci,co,ks,pad,ups', [(32, 20, 3, 1, 0), (16, 16, 3, 1, 1), (144, 32, 3, 1, 0), (8, 8, 3, 1, 0), (32, 32, 1, 0, 0), (16, 16, 4, 0, 0)])
def test_nonsquare_conv(rz, N, H, W, ci, co, ks, pad, ups):
    ran = conv_case(rz, N, H, W, ci, co, ks, pad, ups, may_refuse=True)
    assert ran or ks == 4          # the 4x4 kernel serves the 4x4 and 1x1 maps it exists for (PG_E_UNSUP on an 8x16 map); 3x3 and 1x1 must run


@pytest.mark.parametrize('N,H,W', NONSQUARE)
@pytest.mark.parametrize('cand', [-1, 3, 6])
def test_nonsquare_fused_epilogues(rz, N, H, W, cand):
    ran_pool = pool_case(rz, N, H, W, 32, 16, cand)
    ran_unpool = unpool_case(rz, N, H, W, 32, 16, cand)
    assert (ran_pool and ran_unpool) or cand != -1             # the built-in choice refuses nothing; a forced candidate may not exist
    pg._lib.load().pg_debug_set_tuning(0, -1)
    pixelnorm_conv_case(rz, N, H, W, 12, 20)
    # pg_conv2d_unpooled_nhwc: "Implemented for the 8/16-channel layers of the 512^2/1024^2 stages (block-MFMA kernels); PG_E_UNSUP otherwise"
    unpooled_case(rz, N, H, W, 8, 8)


@pytest.mark.parametrize('N,H,W', NONSQUARE_STRIP)
@pytest.mark.parametrize('ci', [8, 16])
@pytest.mark.parametrize('twin', [False, True])
def test_nonsquare_row_streaming(rz, N, H, W, ci, twin):
    lib = pg._lib.load()
    if twin:
        assert lib.pg_debug_set_tuning(3, 20) == 0 and lib.pg_debug_set_tuning(1, 20) == 0
    conv_case(rz, N, H, W, ci, 8, 3, 1, 0)
    pixelnorm_conv_case(rz, N, H, W, ci, 8)
    assert pool_case(rz, N, H, W, ci, 8, -1)
    assert unpooled_case(rz, N, H, W, ci, 8)                   # strip-sized 8 / 16-channel maps: the layers the entry points exist for


@pytest.mark.parametrize('N,H,W', NONSQUARE_STRIP)
def test_nonsquare_rgb_fused(rz, N, H, W):
    assert rgb_fused_case(rz, N, H, W, 3)                      # "W % 64 == 0, H % 16 == 0": both maps qualify


@pytest.mark.parametrize('N,H,W', NONSQUARE + [(1, 32, 64), (1, 64, 32)])
@pytest.mark.parametrize('variant', [0, 20, 21])
def test_nonsquare_winograd(rz, N, H, W, variant):
    lib = pg._lib.load()
    assert lib.pg_debug_set_wino(variant) == 0
    ci, co = (64, 36) if H * W <= 128 else (16, 32)
    assert wino_case(rz, N, H, W, ci, co, 0)                   # "H, W powers of two >= 8": the forward runs on all four maps
    assert wino_case(rz, N, H, W, ci, co, 1, epilogues=False)
    assert wino_pn_case(rz, N, H, W, 16, 24, 0)
    assert wino_wgrad_case(rz, N, H, W, ci, co, 0) == (W >= 16)      # "H >= 8, W >= 16": W = 8 is refused, the rest must run


@pytest.mark.parametrize('N,H,W', NONSQUARE + [(1, 4, 256), (1, 256, 4)])
def test_nonsquare_rgb_pool_upsample(rz, N, H, W):
    rgb_case(rz, N, 3, H, W, 8 if H * W >= 1024 else 12)
    pool_up_case(rz, N, H, W, 12)


# --------------------------------------------------------------------------------------------- metrics and I/O
# pg_swd_channel_stats / pg_swd_l1: "partials: PG_SWD_REDUCE_BLOCKS * 6 doubles of scratch" -- scratch, as many as the launch has workgroups
SWD_PARTIALS = ('_swd_partials:0',)
# uint8 image outputs: 0xA5 is a legal value, so only their bands are checked ("run with two sentinels or check the bands only")
U8_IMAGES = ('image_grid_u8:0', 'pyramid_level_u8:0')


def test_swd_entry_points(rz):
    import swd_ref
    G = rz.guard
    gen = lambda s: torch.Generator().manual_seed(s)
    x = torch.rand((2, 3, 32, 32), generator=gen(32)) * 2 - 1
    got = ops.lap_pyramid(G(x)); chk(rz)
    for g, r in zip(got, swd_ref.lap_pyramid(x)):
        assert float((g.cpu() - r).abs().max()) <= 2e-6
    S, N, P, off = 16, 3, 5, 4
    level = torch.randn(N, 3, S, S, generator=gen(S))
    centres = torch.randint(3, S - 3, (N * P, 2), generator=gen(S + 1), dtype=torch.int32)
    centres[0], centres[4], centres[7], centres[14] = torch.tensor([[3, 3], [S - 4, 3], [3, S - 4], [S - 4, S - 4]], dtype=torch.int32)
    rows = off + N * P + 3
    out = G(torch.full((rows, 147), -7.5), inplace=True, name='descriptors')
    ops.swd_gather(G(level), G(centres), P, out, off); chk(rz)
    assert torch.equal(out[off:off + N * P].cpu(), swd_ref.descriptors(level, centres, P).reshape(N * P, 147))
    assert bool((out[:off] == -7.5).all()) and bool((out[off + N * P:] == -7.5).all())
    M = 7
    desc = torch.randn(M, 3, 7, 7, generator=gen(M)) * torch.tensor([0.5, 2.0, 1.0]).view(1, 3, 1, 1) + torch.tensor([3.0, -1.0, 0.1]).view(1, 3, 1, 1)
    d = G(desc.reshape(M, 147).contiguous(), inplace=True)
    ops.swd_normalize_(d); chk(rz, may_stay_unwritten=SWD_PARTIALS)
    assert float((d.cpu().double() - swd_ref.normalize(desc.double())).abs().max()) <= 1e-5
    for M, K in ((1, 1), (37, 64)):
        desc = torch.randn(M, 147, generator=gen(1000 * M + K))
        dirs = torch.randn(147, K, generator=gen(K), dtype=torch.float64)
        dirs = (dirs / dirs.pow(2).sum(dim=0, keepdim=True).sqrt()).float().contiguous()
        got = ops.swd_project(G(desc), G(dirs)); chk(rz)
        assert float((got.cpu().double() - (desc.double() @ dirs.double()).t()).abs().max()) <= 2e-5
    for M in (1, 127, ops.SWD_SORT_LDS_ROW + 1):                # one workgroup in LDS | runs + a merge pass through the scratch
        rowsx = torch.randn(3, M, generator=gen(M))
        b = G(rowsx, inplace=True)
        ops.swd_sort_rows_(b); chk(rz)
        assert torch.equal(b.cpu(), rowsx.sort(dim=1)[0])
    a, b = torch.randn(1000, generator=gen(1)), torch.randn(1000, generator=gen(2))
    got = ops.swd_l1(G(a), G(b)); chk(rz, may_stay_unwritten=SWD_PARTIALS)
    ref64 = float((a.double() - b.double()).abs().mean())
    assert abs(float(got) - ref64) / ref64 <= 1e-6


def test_io_step_entry_points(rz):
    import os
    import numpy as np
    from conftest import GOLDEN
    fx = np.load(os.path.join(GOLDEN, 'io_steps.npz'))
    G = rz.guard
    out = ops.real_prepare_u8(G(torch.from_numpy(fx['real/a/in'])), float(fx['real/a/alpha'])); chk(rz)
    assert np.array_equal(out.cpu().numpy(), fx['real/a/out'])
    imgs, res = fx['grid/g1/in'], int(fx['grid/g1/res'])
    grid = ops.image_grid_u8(G(torch.from_numpy(imgs)), (-1, 1), 1 if res < 0 else res // imgs.shape[-1]); chk(rz, may_stay_unwritten=U8_IMAGES)
    assert np.array_equal(grid.cpu().numpy().reshape(fx['grid/g1/out'].shape), fx['grid/g1/out'])
    out = ops.pyramid_level_u8(G(torch.from_numpy(fx['pyr/p1/in'])), int(fx['pyr/p1/diff'])); chk(rz, may_stay_unwritten=U8_IMAGES)
    assert np.array_equal(out.cpu().numpy(), fx['pyr/p1/out'])


def test_msssim_entry_points(rz):
    """pg_msssim_scale (modes 2 / 1 / 0, with and without the pooled outputs) and pg_msssim_finish through ops.msssim_pairs, whose
    work buffers (MSSSIMScratch: pooled images, fp64 partials) and fp64 results all come from the recording allocator; inputs and
    fp64 reference of tests/test_msssim_gpu.py at its two smallest shapes (one scale; two scales = a pooled level), its bound."""
    import test_msssim_gpu as TM
    for shape in ((1, 1, 16), (3, 3, 32)):
        a, b = TM.inputs(shape, 'smooth')
        ad, bd = rz.guard(a), rz.guard(b)
        for quantize in (True, False):
            want_v, want_t = TM.reference(shape, 'smooth', quantize)
            values, terms = ops.msssim_pairs(ad, bd, quantize=quantize)
            chk(rz)                                            # every partial, pooled pixel, term and value is written: no exemption
            assert values.dtype == torch.float64
            assert max(TM._err(values, want_v), TM._err(terms, want_t)) <= TM.BOUND


def test_griffinlim_entry_points(rz):
    """pg_gl_spectrum_f64, pg_gl_pieces_f64 (with a start and, x == NULL, the 'reallog' form), pg_overlap_add_f64 and
    pg_wave_normalize_f32 between fp64 guard bands; cases, oracle and bounds of tests/test_griffinlim_gpu.py at its two smallest
    shapes (n_fft 8 < hop: samples no frame covers; odd hop, many frames per sample)."""
    import numpy as np
    import test_griffinlim_gpu as TG
    G = rz.guard
    t = lambda a: torch.from_numpy(np.array(a, order='C'))
    for (H, hop, batch) in TG.CASES[:2]:
        img, x0, mag, ref_pieces = TG._case(H, hop, batch)
        imgd, x0d = G(t(img)), G(t(x0))
        spec = ops.gl_spectrum(imgd, 'abslog', (-1, 1)); chk(rz)
        assert np.array_equal(spec.cpu().numpy(), mag.transpose(0, 2, 1))
        specd = G(t(mag.transpose(0, 2, 1)))
        pieces = ops.gl_pieces(x0d, specd, hop); chk(rz)
        TG._close(pieces, ref_pieces, 'guarded pieces H=%d hop=%d' % (H, hop))
        want = np.stack([TG._host_overlap_add(p, hop) for p in ref_pieces])
        got = ops.overlap_add(G(t(ref_pieces)), hop); chk(rz)
        assert np.array_equal(got.cpu().numpy(), want)
        real = ops.gl_pieces(None, specd, hop); chk(rz)                            # x == NULL: spec taken as a real spectrum
        win = TG.oss.hann_periodic(2 * H) * (2.0 / 3.0)
        TG._close(real, np.stack([np.stack([win * np.fft.irfft(mag[b][:, f].astype(np.complex128), 2 * H) for f in range(H)]) for b in range(batch)]),
                  'guarded real-spectrum pieces H=%d' % H)
        ref = np.stack([TG.oss.griffin_lim(mag[b], hop, 1, TG._Starts(x0[b])) for b in range(batch)])
        sig = ops.griffin_lim(imgd, x0d, hop, 1); chk(rz)
        TG._close(sig, ref, 'guarded griffin_lim(1) H=%d hop=%d' % (H, hop))
        for repeat in (1, 2):
            wav = ops.wave_normalize(G(t(ref)), repeat); chk(rz)                   # (the peak scratch is batch doubles, all written)
            assert np.array_equal(wav.cpu().numpy(), np.stack([(s_ / np.abs(s_).max()).repeat(repeat).astype(np.float32) for s_ in ref]))


@pytest.mark.parametrize('mode,n_fft,hop,stereo', [('abslog', 256, 128, False), ('reallog', 256, 64, True), ('raw', 0, 0, True)])
def test_sound_entry_points(rz, mode, n_fft, hop, stereo):
    """pg_stft_image (both modes) / pg_mono_f32, pg_minmax_f32 and pg_stretch_to_u8 through ops.spectrogram_u8, and pg_stft_abslog by
    itself; smallest cases, oracle and bound of tests/test_sound_steps.py (at most 1 LSB apart on < 0.1 % / 0.2 % of the pixels).
    The uint8 image may hold any value: only its bands are checked."""
    import numpy as np
    import test_sound_steps as TS
    n = hop * (n_fft // 2 + 3) + 11 if mode != 'raw' else 70000
    y = TS._chirp(n, seed=n_fft if mode == 'abslog' else 17)
    if stereo:
        y = np.stack([y, TS._chirp(n, seed=7)], axis=1)
    ref = TS.oss.spectrogram_image(y, n_fft, hop, img_mode=mode)
    yd = rz.guard(torch.from_numpy(y))
    got = ops.spectrogram_u8(yd, n_fft or 1024, hop or 128, img_mode=mode)
    chk(rz, may_stay_unwritten=(got,))
    diff = np.abs(got.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
    assert got.shape == ref.shape and diff.max() <= 1 and (diff > 0).mean() < (1e-3 if mode == 'abslog' else 2e-3)
    if mode == 'abslog':                                       # pg_stft_abslog == pg_stft_image(PG_SOUND_ABSLOG), bit for bit
        side = n_fft // 2
        a, b = rz.out((side, side), name='stft_abslog'), rz.out((side, side), name='stft_image')
        pg._lib.call('pg_stft_abslog', yd.data_ptr(), n, 1, a.data_ptr(), n_fft, hop, side, side, ops._stream())
        pg._lib.call('pg_stft_image', yd.data_ptr(), n, 1, b.data_ptr(), n_fft, hop, side, side, 0, ops._stream())
        chk(rz, keep_outputs=True)
        assert torch.equal(a, b)
        rz.discard_outputs()


# ------------------------------------------------------------------------------------------------------- coverage
# From a reading of the dispatchers: every __global__ conv kernel of csrc/conv_igemm.hip (dispatch_conv / launch_conv, launch_ksplit),
# conv_thin.hip (dispatch_thin), conv_k4.hip (launch_k4_conv, launch_k4_wgrad), conv_wgrad.hip (the weight-gradient launchers),
# conv_strip.hip (launch_conv_strip, launch_wgrad_strip and the two RGB-fused launchers), conv_wino.hip, conv_wino_strip.hip and
# conv_wino_wgrad.hip whose symbol the pg_debug_last_* calls report.  (conv_epilogue_kernel is the deferred epilogue of a split-K conv_igemm_kernel launch and has no symbol of its own there;
# the weight-transform and pack kernels are covered by test_weight_transforms_batched_in_flat_buffers.)
CONV_FAMILIES = {
    'conv_igemm_kernel', 'conv_ksplit_kernel', 'conv_thin_kernel', 'conv_k4_expand_kernel', 'conv_k4_reduce_kernel',
    'conv_k4_reduce_split_kernel', 'conv_wgrad_kernel', 'conv_k4_wgrad_kernel', 'conv_wgrad_thin_kernel',
    'conv_strip_kernel', 'conv_strip_x_kernel', 'conv_strip_rgb_kernel', 'wgrad_strip_kernel',
    'conv_wino2_kernel', 'conv_wino_strip_kernel', 'conv_wino_wgrad_kernel', 'conv_wino_wgrad_pair_kernel',
}


def test_every_conv_kernel_family_ran_under_the_guards():
    print(sorted(SEEN))
    assert not CONV_FAMILIES - SEEN, 'never launched under the guards: %s' % sorted(CONV_FAMILIES - SEEN)
