"""GPU tier of the kernel distance (csrc/kid.hip, ops.kid_tilesums_f64, metrics.KernelDistance / kid_statistic, plugins.KIDMonitor)
against tests/kid_ref.py.

Integer data that rounds nowhere is compared with ==: whole tiles, and one hot pair at a time, which shows an error of the accumulator
map or of the masks that a whole-tile sum would hide.  Random data is held to a bound that holds for ANY order of the fp64 operations
(tests/kid_ref.pairs_exact derives it from the operation sequence: F additions in the dot product, one multiplication and one addition
in t, two multiplications in k, at most 4096 additions per tile) against math.fsum over the exact products.  Every comparison with a
bound prints its measured maximum as a ratio to the bound before it asserts."""
import functools
import types

import numpy as np
import pytest
import torch

import fd_ref
import kid_ref
from dataset_ref import make_stack

import pggan_amd as pg

pytestmark = pytest.mark.gpu
M_ = pg.metrics
DEV = 'cuda'


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def sums_of(x, y=None, **kw):
    return pg.ops.kid_tilesums_f64(dev(x), dev(y), **kw).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ exact integers
def int_features(M, F, seed):
    return np.random.RandomState(seed).randint(-3, 4, (M, F)).astype(np.float32)


@pytest.mark.parametrize('M,N,F', [(130, 67, 16), (1, 1, 16), (64, 64, 16)])
def test_integer_tile_sums_are_exact(M, N, F):
    """Features in [-3, 3], gamma = coef0 = 1: |g| <= 144, |k| <= 145^3 and a tile sums 4096 of them: every partial sum is an integer
    below 2^53 in any order.  The remainders 2 and 3 of (130, 67) make the last tiles ragged differently in rows and columns."""
    x, y = int_features(M, F, 1), int_features(N, F, 2)
    got = sums_of(x, y, gamma=1.0, coef0=1.0)
    want = kid_ref.tilesums_int(x, y)
    assert got.shape == want.shape == ((M + 63) // 64, (N + 63) // 64) and got.dtype == np.float64
    assert np.array_equal(got, want.astype(np.float64))
    assert np.abs(want).max() < 2 ** 53 and len(set(want.reshape(-1).tolist())) == want.size


@pytest.mark.parametrize('skip', [False, True])
def test_integer_tile_sums_of_the_self_form_are_exact(skip):
    x = int_features(130, 16, 3)
    got = sums_of(x, gamma=1.0, coef0=1.0, skip_diagonal=skip)
    want = kid_ref.tilesums_int(x, skip_diagonal=skip)
    assert got.shape == (3, 3) and np.array_equal(got, want.astype(np.float64)) and np.array_equal(got, got.T)
    if skip:
        full = kid_ref.tilesums_int(x)
        assert (np.diag(full) != np.diag(want)).all() and np.array_equal(np.triu(full, 1), np.triu(want, 1))


# -------------------------------------------------------------------------------------------------------------------- one hot pair
HOT = np.array([3, -2, 1, 0, 2, -3, 1, 1, -1, 2, 0, 3, -2, 1, 2, -1], dtype=np.float32)


@pytest.mark.parametrize('i0,j0', [(0, 0), (15, 16), (16, 15), (31, 32), (32, 31), (63, 64), (64, 63), (47, 48), (128, 65), (129, 66)])
def test_one_hot_pair(i0, j0):
    """x is zero except row i0, y except row j0: every valid pair has k = coef0^3 = 8, the pair (i0, j0) has k = (g + 2)^3, so
    sums[a][b] = 8 (valid pairs of the tile) + (k - 8) in the one tile that holds the pair.  A zero-PADDED row also has k = 8: a mask
    applied before the kernel function, or not at all, shows in the ragged tiles."""
    M, N, F = 130, 67, 16
    x, y = np.zeros((M, F), dtype=np.float32), np.zeros((N, F), dtype=np.float32)
    x[i0], y[j0] = HOT, HOT[::-1] + 1
    got = sums_of(x, y, gamma=1.0, coef0=2.0)
    rows, cols = np.minimum(64, M - 64 * np.arange(3)), np.minimum(64, N - 64 * np.arange(2))
    want = 8.0 * np.outer(rows, cols)
    g = int(HOT.dot(HOT[::-1] + 1))
    want[i0 // 64, j0 // 64] += (g + 2) ** 3 - 8
    assert g != 0 and np.array_equal(got, want)
    assert np.array_equal(want, kid_ref.tilesums_int(x, y, 1, 2).astype(np.float64))


@pytest.mark.parametrize('i0,j0', [(0, 0), (64, 64), (129, 129), (15, 16), (31, 32), (63, 64), (129, 128), (5, 129)])
@pytest.mark.parametrize('skip', [False, True])
def test_hot_rows_of_the_self_form(i0, j0, skip):
    """The self form with rows i0 and j0 hot (one row where they are equal): with skip_diagonal the pairs (i0, i0) and (j0, j0) leave,
    (i0, j0) and (j0, i0) stay."""
    M, F = 130, 16
    x = np.zeros((M, F), dtype=np.float32)
    x[i0] = HOT
    x[j0] = HOT[::-1] + 1 if j0 != i0 else HOT
    got = sums_of(x, gamma=1.0, coef0=2.0, skip_diagonal=skip)
    want = kid_ref.tilesums_int(x, None, 1, 2, skip_diagonal=skip).astype(np.float64)
    assert np.array_equal(got, want) and np.array_equal(got, got.T)
    rows = np.minimum(64, M - 64 * np.arange(3))
    plain = 8.0 * (np.outer(rows, rows) - (np.diag(rows) if skip else 0))
    assert (want != plain).sum() == (0 if skip and i0 == j0 else 1 if i0 // 64 == j0 // 64 else 2 if skip else 4)


# --------------------------------------------------------------------------------------------------------------- the summation bound
@functools.lru_cache(maxsize=None)
def bound_case(M, N, F, offset):
    """(x, y, sums, bound) with y None for the self form (N = 0); shared between the tests and never modified."""
    rs = np.random.RandomState(1000 * F + M + N)
    scale = np.linspace(0.05, 0.6, F)                                             # the embedding's features are means of 16 unit-RMS values
    x = (rs.randn(M, F) * scale + 0.2 * rs.randn(1, F) + offset).astype(np.float32)
    y = (rs.randn(N, F) * scale + 0.2 * rs.randn(1, F) + offset).astype(np.float32) if N else None
    return (x, y) + kid_ref.tilesums_exact(x, y, skip_diagonal=not N)


@pytest.mark.parametrize('offset', [0.0, 100.0])
@pytest.mark.parametrize('M,N,F', [(2, 2, 16), (67, 130, 48), (300, 513, 128), (513, 0, 128)])
def test_tile_sums_within_the_summation_bound(M, N, F, offset):
    """|device - reference| <= bound per tile, the bound of tests/kid_ref.pairs_exact summed over the pairs of the tile:
        1.01 sum_pairs [ e_k(F) + e_k(1) + 4097 U T^3 ],  e_k(c) = 3 T^2 (c U |gamma| G + 2 U T) + 2 U T^3,  T = |gamma| G + |coef0|,
    G = sum_f |x_f y_f|, U = 2^-53: F additions in g on the device (1 rounding in the reference), one multiplication and one addition in
    t, two multiplications in k, at most 4096 additions per tile (1 rounding in the reference).  N = 0: the self form with
    skip_diagonal, which is also symmetric bit for bit.  Two calls give the same bits."""
    x, y, want, bound = bound_case(M, N, F, offset)
    xd, yd = dev(x), dev(y)
    got_d = pg.ops.kid_tilesums_f64(xd, yd, skip_diagonal=not N)
    got = got_d.cpu().numpy()
    err = np.abs(got - want)
    some = bound > 0                          # (the last tile of the self form of 513 rows holds the pair (512, 512) alone: 0 within 0)
    print('tile sums (%d, %d, %d) offset %g: largest error / bound = %.4f (largest error %.3e, largest sum %.3e)'
          % (M, N, F, offset, (err[some] / bound[some]).max(), err.max(), np.abs(want).max()))
    assert got.shape == want.shape and np.isfinite(got).all() and (err <= bound).all()
    assert torch.equal(pg.ops.kid_tilesums_f64(xd, yd, skip_diagonal=not N), got_d)
    if not N:
        assert np.array_equal(got, got.T)
        out = torch.full_like(got_d, -1.0)
        assert pg.ops.kid_tilesums_f64(xd, skip_diagonal=True, out=out) is out and torch.equal(out, got_d)
        with_diag = pg.ops.kid_tilesums_f64(xd).cpu().numpy()
        assert np.array_equal(np.triu(with_diag, 1), np.triu(got, 1)) and (np.diag(with_diag) > np.diag(got)).all()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    z = lambda *shape: torch.zeros(shape, device=DEV)
    for call in (lambda: pg.ops.kid_tilesums_f64(z(8, 24)), lambda: pg.ops.kid_tilesums_f64(z(8, 528)),
                 lambda: pg.ops.kid_tilesums_f64(z(8, 16), z(8, 16), skip_diagonal=True), lambda: pg.ops.kid_tilesums_f64(z(0, 16)),
                 lambda: pg.ops.kid_tilesums_f64(z(8, 16), z(0, 16)), lambda: pg.ops.kid_tilesums_f64(z(8, 16), z(8, 32)),
                 lambda: pg.ops.kid_tilesums_f64(z(8, 16).double()), lambda: pg.ops.kid_tilesums_f64(z(8, 16), out=z(1, 1))):
        with pytest.raises(ValueError):
            call()
    x, out = z(9, 16), torch.zeros(2, dtype=torch.float64, device=DEV)
    fn, stream, C = pg._lib.load().pg_kid_tilesums_f64, pg.ops._stream(), pg._lib.CONSTANTS
    assert fn(x.data_ptr() + 4, 8, None, 8, 16, 1.0, 1.0, 0, out.data_ptr(), stream) == C['PG_E_ALIGN']      # before any launch
    assert fn(x.data_ptr(), 8, x.data_ptr() + 8, 8, 16, 1.0, 1.0, 0, out.data_ptr(), stream) == C['PG_E_ALIGN']
    assert fn(x.data_ptr(), 8, x.data_ptr(), 8, 16, 1.0, 1.0, 1, out.data_ptr(), stream) == C['PG_E_ARG']
    assert fn(x.data_ptr(), 8, None, 8, 24, 1.0, 1.0, 0, out.data_ptr(), stream) == C['PG_E_ARG']
    assert fn(x.data_ptr(), 0, None, 0, 16, 1.0, 1.0, 0, out.data_ptr(), stream) == C['PG_E_ARG']
    torch.cuda.synchronize()
    assert not out.any()                                                          # nothing was written


# -------------------------------------------------------------------------------------------------------------------------- metric
@pytest.mark.parametrize('n,C,r', [(40, 1, 8), (70, 2, 16)])
def test_metric_against_the_reference_over_its_own_features(n, C, r):
    reals, fakes = fd_ref.box_images(n, C, r, 2, seed=n), fd_ref.box_images(n - 7, C, r, 1, seed=n + 1)
    stack = torch.from_numpy(reals).to(DEV)
    kd = M_.KernelDistance(stack, with_fd=True).fit()
    assert tuple(kd.features.shape) == (n, 128) and kd.features.dtype == torch.float32 and kd.sxx.dtype == torch.float64
    for s in range(0, n - 7, 16):
        kd.feed_u8(torch.from_numpy(fakes[s:s + 16]).to(DEV))
    res = kd.result()
    assert (res['num_real'], res['num_fake'], res['subsets'], res['kid_subset_std']) == (n, n - 7, 0, None)
    fx, fy = kd.features.cpu().numpy(), kd.embedding(torch.from_numpy(fakes).to(DEV)).cpu().numpy()
    (sxx, bxx), (syy, byy), (sxy, bxy) = (kid_ref.tilesums_exact(fx, skip_diagonal=True), kid_ref.tilesums_exact(fy, skip_diagonal=True),
                                          kid_ref.tilesums_exact(fx, fy))
    want = M_.kid_statistic(sxx, syy, sxy, n, n - 7)['kid']
    bound = kid_ref.kid_bound(bxx, byy, bxy, sxx, syy, sxy, n, n - 7)
    print('metric [%d, %d, %d, %d]: kid %.9g, reference %.9g, error / bound = %.4f' % (n, C, r, r, res['kid'], want, abs(res['kid'] - want) / bound))
    assert abs(res['kid'] - want) <= bound
    # the same feeds through a FrechetDistance: exactly its fd
    fd = M_.FrechetDistance(stack).fit()
    for s in range(0, n - 7, 16):
        fd.feed_u8(torch.from_numpy(fakes[s:s + 16]).to(DEV))
    assert {k: res[k] for k in ('fd', 'mean_term', 'cov_term')} == {k: fd.result()[k] for k in ('fd', 'mean_term', 'cov_term')}
    plain = M_.KernelDistance(stack, embedding=kd.embedding).fit()
    plain.feed_u8(torch.from_numpy(fakes).to(DEV))                               # one batch instead of five, no fd: the same kid
    assert plain.result()['kid'] == res['kid'] and 'fd' not in plain.result() and plain.mean is None
    # the fitted reals fed back: the two self forms are the same bits
    kd.reset()
    assert kd.syy is None
    kd.feed_u8(stack.index_select(0, kd.indices.to(DEV)))
    back = kd.result()
    assert torch.equal(kd.syy, kd.sxx) and back['num_fake'] == n
    print('metric [%d, %d, %d, %d]: the reals against themselves: kid %.3e' % (n, C, r, r, back['kid']))
    assert back['kid'] < 0                  # the cross term holds the pairs i == j, the self terms do not: below 0, as the estimator is


def test_metric_with_subsets():
    reals, fakes = fd_ref.box_images(200, 1, 8, 2, seed=5), fd_ref.box_images(150, 1, 8, 1, seed=6)
    kd = M_.KernelDistance(torch.from_numpy(reals).to(DEV), subset_size=64).fit()
    kd.feed_u8(torch.from_numpy(fakes).to(DEV))
    res = kd.result()
    sxx, syy, sxy = kd.sxx.cpu().numpy(), kd.syy.cpu().numpy(), kd.sxy.cpu().numpy()
    per = [sxx[s, s] / (64 * 63.0) + syy[s, s] / (64 * 63.0) - 2.0 * sxy[s, s] / (64.0 * 64) for s in range(2)]
    assert res['subsets'] == 2 and res['kid_subset_mean'] == float(np.mean(per)) and res['kid_subset_std'] == float(np.std(per, ddof=1))


# ------------------------------------------------------------------------------------------------------------------------- monitor
def test_monitor_on_a_tiny_network_through_a_stage_change(deterministic_forward):
    torch.manual_seed(11)
    G = pg.Generator((1, 3, 16, 16), latent_size=32, fmap_base=128, fmap_max=32).to('cuda')
    G.depth = 1
    ds = pg.DeviceImageDataset(make_stack(60, 3, 16, seed=7), model_initial_depth=1)
    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=7000, G=G, g_ema=None)
    g = torch.Generator().manual_seed(5)
    drawn = []

    def sample_fn(n):
        drawn.append(torch.randn(n, 32, generator=g))
        return drawn[-1]

    mon = pg.KIDMonitor(ds, sample_fn, num_samples=40, minibatch=16, kid_ticks=1, with_fd=True)
    mon.register(trainer)
    fits = []
    for depth, resolution in ((1, 8), (1, 8), (2, 16)):
        G.depth = ds.model_depth = depth
        del drawn[:]
        trainer.stats.clear()
        mon.epoch(1)
        st = trainer.stats
        assert set(st) == {'kid', 'fd'} and [z.shape[0] for z in drawn] == [16, 16, 8]
        metric = mon._metric_obj
        assert metric.resolution == resolution and metric.shape == (3, resolution, resolution)
        fits.append(metric.sxx)
        check = M_.KernelDistance(ds, with_fd=True).fit()
        assert torch.equal(check.features, metric.features) and torch.equal(check.sxx, metric.sxx)
        for z in drawn:
            check.feed(G.forward(z.cuda()))
        res = check.result()
        assert st['kid']['val'] == res['kid'] and st['fd']['val'] == res['fd'] and np.isfinite(res['kid']) and res['num_fake'] == 40
    assert fits[0] is fits[1] and fits[1] is not fits[2]                          # refitted once, at the stage change
    small = pg.KIDMonitor(ds, sample_fn, num_samples=2, minibatch=2, kid_ticks=1)   # no floor beyond 2
    small.register(trainer)
    trainer.stats.clear()
    small.epoch(1)
    assert set(trainer.stats) == {'kid'} and np.isfinite(trainer.stats['kid']['val'])
