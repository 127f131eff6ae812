"""CPU tier of the normalisation checks: the fp64 references of tests/norm_ref.py tied to float64 autograd of the plain forward
definitions (adjoints are ``torch.autograd.grad``, tangents a JVP, ``inj`` the gradient of <t, P(h) a>, the minibatch-stddev
Hessian-vector term the gradient of <tx, grad_x(Gs1 sigma)>), the exact-global composition over 2 and 3 ranks, the launch geometry the
bounds count with, and the mutation table: one factor off by 5 % must leave the derived bound at every shape the GPU tier runs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as ref

TOL = 1e-12
SLOPE = ref.f32(0.2)


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b.detach().numpy() if torch.is_tensor(b) else b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= TOL * np.maximum(np.abs(b).max(), 1e-300)))


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _pn(h, eps):
    return h * torch.rsqrt((h * h).mean(-1, keepdim=True) + eps)


def _saved(x):
    """fp32 y, r as a device forward would have saved them (correctly rounded)."""
    y, _, r, _ = ref.pixelnorm_fwd(x)
    return y.astype(np.float32), r.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- geometry
def test_chain_lengths_follow_the_launch_geometry():
    assert [ref.pick_lpp(C) for C in ref.PN_C] == [1, 2, 4, 4, 8, 16, 64, 64, 64, 64]
    assert [ref.pn_chain(C) for C in ref.PN_C] == [4, 5, 6, 6, 7, 8, 10, 10, 14, 18]       # 1, 1, 1, 1, 1, 1, 1, 1, 2, 3 float4 per lane
    assert ref.pn_chain(8, True) == 8 and ref.pn_chain(16, True) == 16 and ref.pn_narrow(8) and ref.pn_narrow(16) and not ref.pn_narrow(12)
    # one turn of the grid-stride loop covers 4096 x 256 / LPP pixels: 131 072 at C = 20 (LPP 8: its last 37 pixels are in the THIRD
    # turn), 16 384 at C = 512 (LPP 64: its last 5 pixels are the second turn)
    assert ref.PN_WRAP == ((2 * 131072 + 37, 20), (16384 + 5, 512)) and all(ref.pn_wraps(P, C) for P, C in ref.PN_WRAP)
    assert not ref.pn_wraps(131072, 20) and not ref.pn_wraps(16384, 512)
    assert not any(ref.pn_wraps(P, C) for P in ref.PN_P for C in ref.PN_C)
    sl = ref.mb_slices(432)                                                                 # (2, 3, 16, 36): 30 slices of 14, one of 12, one empty
    assert [e - b for b, e in sl] == [14] * 30 + [12, 0] and sl[-1] == (432, 432)
    assert [e - b for b, e in ref.mb_slices(16)] == [1] * 16 + [0] * 16                     # (1, 1, 16, 4)
    assert [e - b for b, e in ref.mb_slices(10240)] == [320] * 32                           # (2, 5, 16, 512): two float4 per thread
    assert ref.rows_chain(48) == 11 and ref.rows_chain(272) == 12 and ref.rows_chain(320) == 12
    cap = ref.GRID_CAP * 256
    N, H, W, C = ref.POOL_WRAP_FWD
    assert N * H * W * C // 4 > cap
    N, H, W, C = ref.POOL_WRAP_BWD
    assert N * 4 * H * W * C // 4 > cap and ref.AXPBY_WRAP // 4 > cap and ref.SIGNBYTES_WRAP > 8192 * 256


def test_masks_at_zero_take_the_slope():
    m = np.array([1.0, 0.0, -0.0, -1.0, 1e-45], np.float32)
    assert ref._lrelu_factor(m, 0.2).tolist() == [1.0, SLOPE, SLOPE, SLOPE, 1.0]
    v, e = ref.axpby_mask(np.ones(5, np.float32), mask=m, a=1.0, mask_slope=0.0)
    assert v.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0]


# --------------------------------------------------------------------------------------------------------- PixelNorm and autograd
@pytest.mark.parametrize('P,C', [(1, 4), (5, 12), (37, 16), (37, 144), (5, 528)])
def test_pixelnorm_formulas_are_autograd_of_the_forward(P, C):
    x, gy, t, a = (v.astype(np.float64) for v in ref.pn_inputs(P, C))
    eps = ref.f32(1e-8)
    z = _t(x, True)
    h = F.leaky_relu(z, SLOPE)
    y = _pn(h, eps)
    want_y, _, want_r, _ = ref.pixelnorm_fwd(h.detach().numpy(), eps)
    assert _close(want_y, y) and _close(want_r, torch.rsqrt((h * h).mean(-1) + eps))
    gz, = torch.autograd.grad(y, z, _t(gy), retain_graph=True)
    got, bound = ref.pixelnorm_lrelu_bwd(gy, y.detach().numpy(), want_r, SLOPE)
    assert _close(got, gz) and np.all(bound >= 0)
    gz0, = torch.autograd.grad(h, z, _t(gy), retain_graph=True)                                        # r absent: the LeakyReLU alone
    got, bound = ref.pixelnorm_lrelu_bwd(gy, h.detach().numpy(), None, SLOPE)
    assert _close(got, gz0) and np.all(bound[h.detach().numpy() > 0] == 0)
    # tangent and injection at the PixelNorm input h
    hh = h.detach().clone().requires_grad_(True)
    yy = _pn(hh, eps)
    _, ty = torch.autograd.functional.jvp(lambda v: _pn(v, eps), hh.detach(), _t(t))
    Pa, = torch.autograd.grad(yy, hh, _t(a), create_graph=True)
    inj, = torch.autograd.grad((_t(t) * Pa).sum(), hh)
    got_ty, _, got_inj, b_inj = ref.pixelnorm_tangent(t, yy.detach().numpy(), want_r, a)
    assert _close(got_ty, ty) and _close(got_inj, inj) and np.all(b_inj >= 0)
    # ... and the adjoint that takes the injection: d/dz [<gy, y(z)> + <inj, h(z)>]
    gzi, = torch.autograd.grad((_t(gy) * y).sum() + (inj.detach() * h).sum(), z)
    got, _ = ref.pixelnorm_lrelu_bwd(gy, y.detach().numpy(), want_r, SLOPE, inj=inj.numpy())
    assert _close(got, gzi)


# ---------------------------------------------------------------------------------------------------- minibatch stddev and autograd
def _mb_forward(x, G, cp):
    """The plain definition (network.py:174-187 on NHWC): one sigma per group, in channel C of a zero-padded copy."""
    NB, C = x.shape[0], x.shape[-1]
    xg = x.reshape(G, -1)
    mu = xg.mean(1, keepdim=True)
    sigma = torch.sqrt(((xg - mu) ** 2).mean(1) + ref.MB_EPS)
    pad = torch.zeros(x.shape[:-1] + (cp - C,), dtype=x.dtype)
    pad[..., 0] = 1
    return torch.cat([x, pad * sigma.repeat_interleave(NB // G).reshape((NB,) + (1,) * (x.dim() - 1))], -1), mu.reshape(-1), sigma


@pytest.mark.parametrize('case', [(1, 4, 16, 16), (2, 3, 16, 36), (1, 1, 16, 4), (2, 17, 16, 8)])
@pytest.mark.parametrize('cond', [False, True])
def test_mbstd_formulas_are_autograd_of_the_forward(case, cond):
    G, n, HW, C = case
    cp = C + 16
    x, tx, gy, gf = (v.astype(np.float64) for v in ref.mb_inputs(G, n, HW, C, cond))
    z = _t(x, True)
    xx = F.leaky_relu(z, SLOPE)
    y, mu, sigma = _mb_forward(xx, G, cp)
    xh = xx.detach().numpy()
    want_y, _, w_mu, e_mu, w_sigma, e_sigma = ref.mbstd_fwd(xh, G, cp)
    assert _close(want_y, y) and _close(w_mu, mu) and _close(w_sigma, sigma) and np.all(e_mu > 0) and np.all(e_sigma > 0)
    assert not want_y[..., C + 1:].any()
    stats = np.stack([w_mu, w_sigma], 1)
    _, ty = torch.autograd.functional.jvp(lambda v: _mb_forward(v, G, cp)[0], xx.detach(), _t(tx))
    got_ty, _, tmean, _, dot, _ = ref.mbstd_tangent(tx, stats, G, cp, [(xh, tx)])
    assert _close(got_ty, ty) and _close(tmean, tx.reshape(G, -1).mean(1))
    assert _close(dot, ((xh.reshape(G, -1) - w_mu[:, None]) * tx.reshape(G, -1)).sum(1))
    tstats = np.stack([tmean, dot], 1)
    # adjoint, with and without the LeakyReLU mask of the layer below
    gz, = torch.autograd.grad(y, z, _t(gy), retain_graph=True)
    assert _close(ref.mbstd_bwd(gy, xh, stats, G, True, SLOPE)[0], gz)
    x0 = xx.detach().clone().requires_grad_(True)
    y0, _, sigma0 = _mb_forward(x0, G, cp)
    gx, = torch.autograd.grad(y0, x0, _t(gy), retain_graph=True)
    assert _close(ref.mbstd_bwd(gy, xh, stats, G, False)[0], gx)
    # Hessian-vector term: gradient of <tx, grad_x(Gs1 sigma)>
    Gs1 = _t(gf[..., C].reshape(G, -1).sum(1))
    g1, = torch.autograd.grad((Gs1 * sigma0).sum(), x0, create_graph=True)
    hvp, = torch.autograd.grad((_t(tx) * g1).sum(), x0)
    got = ref.mbstd_bwd(None, xh, stats, G, False, tx=tx, tstats=tstats, gy_first=gf)[0]
    assert _close(got, hvp)
    assert _close(ref.mbstd_bwd(gy, xh, stats, G, False, tx=tx, tstats=tstats, gy_first=gf)[0], gx + hvp)
    assert _close(ref.mbstd_bwd(gy, xh, stats, G, True, SLOPE, tx=tx, tstats=tstats, gy_first=gf)[0],
                  (gx + hvp) * _t(ref._lrelu_factor(xh, SLOPE)))


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('case', ref.MB_CASES)
def test_exact_global_composition_equals_the_single_process_reference(case, world):
    G, n, HW, C = case
    n, cp = n * world, C + 16
    x, tx, gy, gf = ref.mb_inputs(G, n, HW, C)
    idx = ref.shard_rows(G, n, world)
    _, _, mu, _, sigma, _ = ref.mbstd_fwd(x, G, cp)
    stats = np.stack([mu, sigma], 1)
    ty, _, tmean, _, dot, _ = ref.mbstd_tangent(tx, stats, G, cp, [(x, tx)])
    tstats = np.stack([tmean, dot], 1)
    shards = [x[i] for i in idx]
    gsums = sum(np.stack([ref.mbstd_gsum(gy[i], G, C)[0], ref.mbstd_gsum(gf[i], G, C)[0]], 1) for i in idx)
    assert _close(gsums[:, 0], ref.mbstd_gsum(gy, G, C)[0]) and _close(gsums[:, 1], ref.mbstd_gsum(gf, G, C)[0])
    for r, i in enumerate(idx):
        y_r, _, mu_r, _, sigma_r, _ = ref.mbstd_fwd(x[i], G, cp, shards=shards)
        assert _close(mu_r, mu) and _close(sigma_r, sigma) and _close(y_r[..., C], np.repeat(sigma, n // world).reshape(-1, 1, 1) + 0 * y_r[..., C])
        ty_r, _, tm_r, _, dot_r, _ = ref.mbstd_tangent(tx[i], stats, G, cp, [(x[j], tx[j]) for j in idx])
        assert _close(ty_r, ty[i]) and _close(tm_r, tmean) and _close(dot_r, dot)
        for am in (False, True):
            for use_gy, use_tx in ((True, False), (True, True), (False, True)):
                kw = dict(tx=tx, tstats=tstats, gy_first=gf) if use_tx else {}
                whole = ref.mbstd_bwd(gy if use_gy else None, x, stats, G, am, SLOPE, **kw)[0]
                kw = dict(tx=tx[i], tstats=tstats, gy_first=gf[i]) if use_tx else {}
                part = ref.mbstd_bwd(gy[i] if use_gy else None, x[i], stats, G, am, SLOPE, gsums=gsums, nranks=world, **kw)[0]
                assert _close(part, whole[i])


def test_sigma_bound_at_a_large_mean_rejects_a_one_pass_variance():
    """x = 30 + 0.01 noise: the two-pass slice means and Chan's merge keep sigma to the derived 2.2e-4 relative (the bound's own figure,
    asserted below); sum and sum of squares in fp32, however carefully added, lose sigma at the first rounding of 900."""
    G, n, HW, C = 2, 5, 16, 512
    x = ref.mb_inputs(G, n, HW, C, cond=True)[0]
    mu, e_mu, sigma, e_sigma = ref.mbstd_stats([x], G)
    assert np.all(np.abs(sigma - 0.01) < 1e-4) and np.all(e_sigma / sigma < 2.2e-4) and np.all(e_mu < 7e-5)
    xg = x.reshape(G, -1)
    M = np.float32(xg.shape[1])
    mean = np.sum(xg, 1, dtype=np.float32) / M                                   # (numpy adds pairwise: the kindest one-pass order)
    one_pass = np.sqrt(np.maximum(np.sum(xg * xg, 1, dtype=np.float32) / M - mean * mean, np.float32(0)) + np.float32(1e-8))
    assert np.all(np.abs(one_pass.astype(np.float64) - sigma) > e_sigma)


# --------------------------------------------------------------------------------------------------------------- pool and autograd
@pytest.mark.parametrize('case', ref.POOL_CASES)
def test_pool_formulas_are_autograd_of_the_forward(case):
    x, other, gy, mask = (v.astype(np.float64) for v in ref.pool_inputs(*case))
    a, b = ref.f32(0.3), ref.f32(0.7)
    nchw = lambda v: v.permute(0, 3, 1, 2)
    nhwc = lambda v: v.permute(0, 2, 3, 1)
    xt = _t(x, True)
    pooled = nhwc(F.avg_pool2d(nchw(xt), 2))
    assert _close(ref.avgpool2_fwd(x)[0], pooled) and _close(ref.avgpool2_fwd(x, a=a)[0], a * pooled)
    assert _close(ref.avgpool2_fwd(x, other, a, b)[0], a * pooled + b * _t(other))
    m = _t(mask, True)
    gx, = torch.autograd.grad(nhwc(F.avg_pool2d(nchw(F.leaky_relu(m, SLOPE)), 2)), m, _t(gy) * a)     # pool adjoint through the LeakyReLU below
    assert _close(ref.avgpool2_bwd(gy, mask, a, SLOPE)[0], gx)
    gx, = torch.autograd.grad(pooled, xt, _t(gy))
    assert _close(ref.avgpool2_bwd(gy)[0], gx)
    c = _t(gy, True)
    up = nhwc(F.interpolate(nchw(c), scale_factor=2, mode='nearest'))
    gc, = torch.autograd.grad(up, c, _t(x))
    assert _close(ref.upsample2_bwd(x)[0], gc)
    gm, = torch.autograd.grad(F.leaky_relu(m, SLOPE), m, a * _t(x) + b * _t(mask))
    assert _close(ref.axpby_mask(x, mask, mask, a, b, SLOPE)[0], gm) and _close(ref.axpby_mask(x, a=a)[0], a * x)


# ----------------------------------------------------------------------------------------------------------------- mutation table
def _rejected(mutated, value, bound):
    return ref.ratio(mutated, value, bound)[0] > 1.0


def _pixelnorm_mutations(P, C):
    x, gy, t, a = ref.pn_inputs(P, C)
    y, r = _saved(x)
    v, b = ref.pixelnorm_lrelu_bwd(gy, y, r, 0.2)
    assert _rejected(ref.pixelnorm_lrelu_bwd(gy, y, r, 0.2, mutate='proj')[0], v, b), ('proj', P, C)
    ty, b_ty, inj, b_inj = ref.pixelnorm_tangent(t, y, r, a)
    for which in ('k_y', 'kp'):
        assert _rejected(ref.pixelnorm_tangent(t, y, r, a, mutate=which)[2], inj, b_inj), (which, P, C)
    inj32 = inj.astype(np.float32)
    v, b = ref.pixelnorm_lrelu_bwd(gy, y, r, 0.2, inj=inj32)
    assert _rejected(ref.pixelnorm_lrelu_bwd(gy, y, r, 0.2, inj=inj32, mutate='inj')[0], v, b), ('inj', P, C)
    assert _rejected(ref.pixelnorm_lrelu_bwd(gy, y, r, 0.2, inj=inj32, mutate='proj')[0], v, b), ('proj with inj', P, C)


@pytest.mark.parametrize('C', ref.PN_C)
def test_five_percent_leaves_the_pixelnorm_bounds(C):
    for P in ref.PN_P:
        _pixelnorm_mutations(P, C)


@pytest.mark.parametrize('P,C', ref.PN_WRAP)
def test_five_percent_leaves_the_pixelnorm_bounds_past_the_grid_cap(P, C):
    _pixelnorm_mutations(P, C)


def _mb_modes(gy, C):
    """full gy; the stddev path alone (pass-through channels 0); the pass-through alone (channel C 0)."""
    std_only, pass_only = gy.copy(), gy.copy()
    std_only[..., :C] = 0
    pass_only[..., C] = 0
    return dict(full=gy, std_only=std_only, pass_only=pass_only)


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('case', ref.MB_CASES)
def test_five_percent_leaves_the_mbstd_bounds(case, world):
    G, n, HW, C = case
    n, cp = n * world, C + 16
    x, tx, gy, gf = ref.mb_inputs(G, n, HW, C)
    _, _, mu, _, sigma, _ = ref.mbstd_fwd(x, G, cp)
    stats = np.stack([mu, sigma], 1).astype(np.float32)
    _, _, tmean, _, dot, _ = ref.mbstd_tangent(tx, stats, G, cp, [(x, tx)])
    tstats = np.stack([tmean, dot], 1).astype(np.float32)
    idx = ref.shard_rows(G, n, world)
    for name, g in _mb_modes(gy, C).items():
        gsums = None if world == 1 else np.stack([ref.mbstd_gsum(g, G, C)[0], ref.mbstd_gsum(gf, G, C)[0]], 1).astype(np.float32)
        for i in idx:
            for am in (False, True):
                for use_gy, use_tx in ((True, False), (True, True), (False, True)):
                    kw = dict(gsums=gsums, nranks=world)
                    if use_tx:
                        kw.update(tx=tx[i], tstats=tstats, gy_first=gf[i])
                    args = (g[i] if use_gy else None, x[i], stats, G, am, 0.2)
                    v, b = ref.mbstd_bwd(*args, **kw)
                    muts = (['std'] if use_gy and name != 'pass_only' else []) + (['hvp_t', 'hvp_x'] if use_tx else [])
                    for which in muts:
                        assert _rejected(ref.mbstd_bwd(*args, mutate=which, **kw)[0], v, b), (which, name, case, world, am, use_gy, use_tx)
                    if name == 'pass_only' and use_gy and not use_tx:              # no stddev path: the pass-through times the mask, exactly
                        assert np.array_equal(v, g[i][..., :C] * (ref._lrelu_factor(x[i], 0.2) if am else 1.0))


def _pool_fwd_mutations(x, other):
    for kw in (dict(), dict(a=0.3), dict(other=other, a=0.3, b=0.7)):
        v, b = ref.avgpool2_fwd(x, **kw)
        assert _rejected(ref.avgpool2_fwd(x, mutate='quarter', **kw)[0], v, b), ('quarter', kw.keys())
    v, b = ref.avgpool2_fwd(x, other, 0.3, 0.7)
    assert _rejected(ref.avgpool2_fwd(x, other, 0.3, 0.7, mutate='b')[0], v, b)


def _pool_bwd_mutations(gy, mask):
    for kw in (dict(), dict(mask=mask, mul=0.3, mask_slope=0.2)):
        v, b = ref.avgpool2_bwd(gy, **kw)
        assert _rejected(ref.avgpool2_bwd(gy, mutate='quarter', **kw)[0], v, b)


def _axpby_mutation(x, other, mask):
    v, b = ref.axpby_mask(x, other, mask, 0.3, 0.7, 0.2)
    assert _rejected(ref.axpby_mask(x, other, mask, 0.3, 0.7, 0.2, mutate='b')[0], v, b)


@pytest.mark.parametrize('case', ref.POOL_CASES)
def test_five_percent_leaves_the_pool_bounds(case):
    x, other, gy, mask = ref.pool_inputs(*case)
    _pool_fwd_mutations(x, other)
    _pool_bwd_mutations(gy, mask)
    _axpby_mutation(x, mask, mask)


def test_five_percent_leaves_the_pool_bounds_past_the_grid_cap():
    x, other, _, _ = ref.pool_inputs(*ref.POOL_WRAP_FWD)
    _pool_fwd_mutations(x, other)
    _, _, gy, mask = ref.pool_inputs(*ref.POOL_WRAP_BWD)
    _pool_bwd_mutations(gy, mask)
    x, other, mask = (ref._randn(50 + i, ref.AXPBY_WRAP) for i in range(3))
    _axpby_mutation(x, other, mask)
