"""PixelNorm, minibatch stddev and the pool / upsample / axpby kernels on the device against fp64 evaluations of their contracts
(tests/norm_ref.py: references and derived per-element bounds; docs/experiments_normalisation_tests.md), at the smallest shapes that reach
each branch of csrc/elementwise.hip: every lanes-per-pixel choice with and without idle lanes, ragged and empty minibatch slices, more
than 256 rows, and one case per kernel past the grid cap (the second turn of the grid-stride loop).  Saved tensors go to the references as
the device produced them and have their own assertion, so each kernel is held to its own rounding.  Assertion: max(err / bound) <= 1 per
output tensor; the ratio and the worst element are printed."""
import numpy as np
import pytest
import torch

import norm_ref as ref

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops
SLOPE = 0.2


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def hold(what, got, want, bound, worst):
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == np.shape(want), (what, got.shape, np.shape(want))
    q, i = ref.ratio(got, want, bound)
    worst.append(q)
    print('    %-46s err / bound %.3f at %s (got %.9g, want %.9g, bound %.3g)'
          % (what, q, tuple(int(k) for k in np.unravel_index(i, got.shape)), got.reshape(-1)[i], np.reshape(want, -1)[i], np.reshape(bound, -1)[i]))
    assert q <= 1.0, (what, q, i)


# ------------------------------------------------------------------------------------------------------------------- PixelNorm
def _pixelnorm(P, C):
    x, gy, t, a = ref.pn_inputs(P, C)
    worst = []
    dx, dgy, dt, da = dev(x), dev(gy), dev(t), dev(a)
    y, r = ops.pixelnorm_fwd(dx)
    want_y, b_y, want_r, b_r = ref.pixelnorm_fwd(x)
    hold('pixelnorm_fwd y', y, want_y, b_y, worst)
    hold('pixelnorm_fwd r', r, want_r, b_r, worst)
    yh, rh = host(y), host(r)
    assert yh[0, 1] == 0 and not np.signbit(yh[0, 1]) and yh[0, 2] == 0 and np.signbit(yh[0, 2])          # 0.0 and -0.0 reach y
    if P >= 5:
        assert not yh[P // 2].any() and abs(rh[P // 2] - 1e4) < 0.01                                       # the all-zero pixel: r = rsqrt(eps)
    x2 = dx.clone()
    y2, r2 = ops.pixelnorm_fwd(x2, inplace=True)
    assert y2.data_ptr() == x2.data_ptr() and torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(r2), _bits(r))
    for with_r in (True, False):
        gz = ops.pixelnorm_lrelu_bwd(dgy, y, r if with_r else None, SLOPE)
        want, bound = ref.pixelnorm_lrelu_bwd(gy, yh, rh if with_r else None, SLOPE)
        hold('pixelnorm_lrelu_bwd%s' % ('' if with_r else ' (no r)'), gz, want, bound, worst)
        g2 = dgy.clone()
        gz2 = ops.pixelnorm_lrelu_bwd(g2, y, r if with_r else None, SLOPE, inplace=True)
        assert gz2.data_ptr() == g2.data_ptr() and torch.equal(_bits(gz2), _bits(gz))
    ty, inj = ops.pixelnorm_tangent(dt, y, r, da)
    want_ty, b_ty, want_inj, b_inj = ref.pixelnorm_tangent(t, yh, rh, a)
    hold('pixelnorm_tangent ty', ty, want_ty, b_ty, worst)
    hold('pixelnorm_tangent inj', inj, want_inj, b_inj, worst)
    gz = ops.pixelnorm_lrelu_bwd(dgy, y, r, SLOPE, inj=inj)
    want, bound = ref.pixelnorm_lrelu_bwd(gy, yh, rh, SLOPE, inj=host(inj))
    hold('pixelnorm_lrelu_bwd_inj', gz, want, bound, worst)
    g2 = dgy.clone()
    assert torch.equal(_bits(ops.pixelnorm_lrelu_bwd(g2, y, r, SLOPE, inplace=True, inj=inj)), _bits(gz))
    assert torch.equal(dx, torch.from_numpy(x).cuda()) and torch.equal(dgy, torch.from_numpy(gy).cuda())   # operands untouched
    print('pixelnorm P %d C %d (LPP %d, chain %d%s): max err / bound %.3f'
          % (P, C, ref.pick_lpp(C), ref.pn_chain(C), ', wraps' if ref.pn_wraps(P, C) else '', max(worst)))


@pytest.mark.parametrize('P', ref.PN_P)
@pytest.mark.parametrize('C', ref.PN_C)
def test_pixelnorm(P, C):
    _pixelnorm(P, C)


@pytest.mark.parametrize('P,C', ref.PN_WRAP)
def test_pixelnorm_past_the_grid_cap(P, C):
    assert ref.pn_wraps(P, C)
    _pixelnorm(P, C)


# ------------------------------------------------------------------------------------------------------------ minibatch stddev
def _gy_modes(gy, C):
    std_only, pass_only = gy.copy(), gy.copy()
    std_only[..., :C] = 0
    pass_only[..., C] = 0
    return (('full', gy), ('std path alone', std_only), ('pass-through alone', pass_only))


def _mbstd(G, n, HW, C, world, cond=False, modes=None):
    n, cp = n * world, C + 16
    x, tx, gy, gf = ref.mb_inputs(G, n, HW, C, cond)
    idx = ref.shard_rows(G, n, world)
    worst = []
    xs, txs = [x[i] for i in idx], [tx[i] for i in idx]
    dxs, dtxs = [dev(v) for v in xs], [dev(v) for v in txs]
    # forward: local entry point, or stats / write with the partial rows stacked rank-major as the all-gather leaves them
    if world == 1:
        outs = [ops.mbstd_fwd(dxs[0], G, cp)]
    else:
        parts = [ops.mbstd_stats(d, G) for d in dxs]
        gathered = torch.stack(parts).contiguous()
        outs = [ops.mbstd_write(d, parts[r].clone(), gathered, cp) for r, d in enumerate(dxs)]
    for r in range(world):
        want_y, b_y, mu, e_mu, sigma, e_sigma = ref.mbstd_fwd(xs[r], G, cp, shards=xs)
        y, st = outs[r]
        hold('mbstd fwd y, rank %d' % r, y, want_y, b_y, worst)
        hold('mbstd mu, rank %d' % r, st[:, 0], mu, e_mu, worst)
        hold('mbstd sigma, rank %d' % r, st[:, 1], sigma, e_sigma, worst)
        assert not bool(y[..., C + 1:].any()) and torch.equal(y[..., :C], dxs[r])
        assert torch.equal(_bits(st[:, :2]), _bits(outs[0][1][:, :2]))                       # mu / sigma bit-identical on every rank
        assert bool((y[..., C] == st[:, 1].repeat_interleave(n // world).view(-1, 1, 1)).all())
    if cond:
        print('    sigma %s, bound / sigma %s' % (sigma, e_sigma / sigma))
    stats = [o[1] for o in outs]
    sth = host(stats[0])[:, :2]
    # tangent
    if world == 1:
        touts = [ops.mbstd_tangent(dxs[0], dtxs[0], stats[0], cp)]
    else:
        tparts = [ops.mbstd_tangent_stats(dxs[r], dtxs[r], stats[r]) for r in range(world)]
        tgath = torch.stack(tparts).contiguous()
        touts = [ops.mbstd_tangent_write(dtxs[r], tparts[r].clone(), tgath, stats[r], cp) for r in range(world)]
    for r in range(world):
        want_ty, b_ty, tmean, e_tmean, dot, e_dot = ref.mbstd_tangent(txs[r], sth, G, cp, list(zip(xs, txs)))
        ty, ts = touts[r]
        hold('mbstd tangent ty, rank %d' % r, ty, want_ty, b_ty, worst)
        hold('mbstd mean(tx), rank %d' % r, ts[:, 0], tmean, e_tmean, worst)
        hold('mbstd <x - mu, tx>, rank %d' % r, ts[:, 1], dot, e_dot, worst)
        assert not bool(ty[..., C + 1:].any()) and torch.equal(ty[..., :C], dtxs[r])
        assert torch.equal(_bits(ts[:, :2]), _bits(touts[0][1][:, :2]))
    tsh = host(touts[0][1])[:, :2]
    # adjoint: full gy, the stddev path alone, the pass-through alone; gy / tx present or absent; with and without the mask
    for name, g in (modes or _gy_modes(gy, C)):
        gs, gfs = [g[i] for i in idx], [gf[i] for i in idx]
        dgs, dgfs = [dev(v) for v in gs], [dev(v) for v in gfs]
        for use_gy, use_tx in ((True, False), (True, True), (False, True)):
            if world > 1:
                sums = []
                for r in range(world):
                    s = ops.mbstd_gsum(dgs[r] if use_gy else None, dgfs[r] if use_tx else None, G, tuple(dxs[r].shape), cp)
                    for k, src in enumerate((gs[r] if use_gy else None, gfs[r] if use_tx else None)):
                        want, bound = ref.mbstd_gsum(src, G, C)
                        hold('mbstd gsum[%d], rank %d' % (k, r), s[:, k], want, bound, worst)
                    sums.append(s)
                gsum = sum(sums)                                                            # the all-reduce: fp32 sums, an operand from here on
            for am in (False, True):
                for r in range(world):
                    kw = dict(tx=dtxs[r], tstats=touts[r][1], gy_first=dgfs[r]) if use_tx else {}
                    rkw = dict(tx=txs[r], tstats=tsh, gy_first=gfs[r]) if use_tx else {}
                    if world == 1:
                        got = ops.mbstd_bwd(dgs[r] if use_gy else None, dxs[r], stats[r], cp, am, SLOPE, **kw)
                    else:
                        got = ops.mbstd_bwd_global(dgs[r] if use_gy else None, dxs[r], stats[r], cp, am, gsum, world, SLOPE, **kw)
                        rkw.update(gsums=host(gsum), nranks=world)
                    want, bound = ref.mbstd_bwd(gs[r] if use_gy else None, xs[r], sth, G, am, SLOPE, **rkw)
                    hold('mbstd bwd %s mask=%d gy=%d hvp=%d rank %d' % (name, am, use_gy, use_tx, r), got, want, bound, worst)
                    if name == 'pass-through alone' and use_gy and not use_tx:              # Gs == 0: gy[..., :C] times the mask, exactly
                        k = torch.where(dxs[r] > 0, 1.0, SLOPE).float() if am else 1.0
                        assert torch.equal(got, dgs[r][..., :C] * k)
    print('mbstd G %d n %d HW %d C %d world %d%s: max err / bound %.3f' % (G, n, HW, C, world, ' x = 30 + 0.01 noise' if cond else '', max(worst)))


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('case', ref.MB_CASES)
def test_mbstd(case, world):
    _mbstd(*case, world)


@pytest.mark.parametrize('world', [1, 2])
def test_mbstd_at_a_large_mean(world):
    """x = 30 + 0.01 noise: the bound (2.1e-4 of sigma in one process, 2.6e-4 over two ranks; tests/test_normalisation_host.py shows that
    a one-pass variance misses it) holds only because every slice takes its own mean first and the partials are merged by Chan's formula."""
    _mbstd(2, 5, 16, 512, world, cond=True)


# ------------------------------------------------------------------------------------------------- pool / upsample / axpby
def _pool(case, worst, refs=None):
    x, other, gy, mask = refs['inputs'] if refs else ref.pool_inputs(*case)
    dx, do, dgy, dm = dev(x), dev(other), dev(gy), dev(mask)
    want = refs or dict(blend=ref.avgpool2_fwd(x, other, 0.3, 0.7), up=ref.upsample2_bwd(x))
    hold('avgpool2_fwd blend', ops.avgpool2_fwd(dx, do, 0.3, 0.7), *want['blend'], worst)
    hold('upsample2_bwd', ops.upsample2_bwd(dx), *want['up'], worst)
    if refs is None:
        hold('avgpool2_fwd', ops.avgpool2_fwd(dx), *ref.avgpool2_fwd(x), worst)
        hold('avgpool2_fwd a', ops.avgpool2_fwd(dx, a=0.3), *ref.avgpool2_fwd(x, a=0.3), worst)
        _pool_bwd(gy, mask, worst)
        hold('axpby_mask', ops.axpby_mask(dx, dm, dm, 0.3, 0.7, SLOPE), *ref.axpby_mask(x, mask, mask, 0.3, 0.7, SLOPE), worst)
        hold('axpby_mask scale', ops.axpby_mask(dx, a=0.3), *ref.axpby_mask(x, a=0.3), worst)
        hold('axpby_mask, mask alone', ops.axpby_mask(dx, mask=dm, a=1.0, mask_slope=0.0), *ref.axpby_mask(x, mask=mask, a=1.0, mask_slope=0.0), worst)


def _pool_bwd(gy, mask, worst, want=None):
    dgy, dm = dev(gy), dev(mask)
    hold('avgpool2_bwd mask', ops.avgpool2_bwd(dgy, dm, 0.3, SLOPE), *(want or ref.avgpool2_bwd(gy, mask, 0.3, SLOPE)), worst)
    if want is None:
        hold('avgpool2_bwd', ops.avgpool2_bwd(dgy), *ref.avgpool2_bwd(gy), worst)
        got = ops.avgpool2_bwd(dgy, dm, 1.0, 0.0)                                            # slope 0: every mask entry <= 0, 0.0 and -0.0 included, gives 0
        assert not bool(got[dm <= 0].any()) and bool((got[dm > 0] != 0).any())


@pytest.mark.parametrize('case', ref.POOL_CASES)
def test_pool_upsample_axpby(case):
    worst = []
    _pool(case, worst)
    print('pool / upsample / axpby %s: max err / bound %.3f' % (case, max(worst)))


@pytest.fixture(scope='module')
def wrap_refs():
    """Inputs and fp64 references of the cases past the grid cap, computed once and never written."""
    x, other, _, _ = ref.pool_inputs(*ref.POOL_WRAP_FWD)
    fwd = dict(inputs=(x, other, None, None), blend=ref.avgpool2_fwd(x, other, 0.3, 0.7), up=ref.upsample2_bwd(x))
    _, _, gy, mask = ref.pool_inputs(*ref.POOL_WRAP_BWD)
    n = ref.AXPBY_WRAP
    ax = tuple(ref._randn(50 + i, n) for i in range(3))
    ax[2][::5] = 0.0
    ax[2][1::10] = -0.0
    return dict(fwd=fwd, bwd=(gy, mask, ref.avgpool2_bwd(gy, mask, 0.3, SLOPE)), axpby=(ax, ref.axpby_mask(ax[0], ax[1], ax[2], 0.3, 0.7, SLOPE)))


def test_pool_past_the_grid_cap(wrap_refs):
    worst = []
    _pool(ref.POOL_WRAP_FWD, worst, wrap_refs['fwd'])
    gy, mask, want = wrap_refs['bwd']
    _pool_bwd(gy, mask, worst, want)
    (x, o, m), want = wrap_refs['axpby']
    hold('axpby_mask', ops.axpby_mask(dev(x), dev(o), dev(m), 0.3, 0.7, SLOPE), *want, worst)
    print('pool / upsample / axpby past the grid cap: max err / bound %.3f' % max(worst))


@pytest.mark.parametrize('nbytes', [1, 37, 1000, ref.SIGNBYTES_WRAP])
def test_signbytes_to_mask(nbytes):
    b = torch.randint(0, 256, (nbytes,), generator=torch.Generator().manual_seed(nbytes), dtype=torch.uint8)
    want = (((b.view(-1, 1).int() >> torch.arange(4, dtype=torch.int32)) & 1) * 2 - 1).float().view(-1)   # bits 0..3; the high nibble is ignored
    got = ops.signbytes_to_mask(b.cuda())
    assert got.shape == (4 * nbytes,) and torch.equal(got.cpu(), want)
