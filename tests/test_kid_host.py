"""The host tier of the kernel distance: the binding of include/pggan_hip_kid.h, metrics.kid_statistic against plain double loops over
all pairs, the reason for the metric -- the estimator is unbiased where the Frechet distance of the same draws is off by a hundred --
the host twin of ops.kid_tilesums_f64 / metrics.KernelDistance (device='cpu') against tests/kid_ref.py, plugins.KIDMonitor on the twin
with a stub trainer, and the argument errors.  Host tests: no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import fd_ref
import kid_ref

import pggan_amd as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = pg.metrics
TOL = 4112                  # roundings on the path of a term of kid_statistic over numpy tile sums (test_statistic_against_double_loops_ragged)


# ------------------------------------------------------------------------------------------------------------------ binding
def test_kid_header_is_derived_completely_and_the_other_tables_are_unchanged():
    _lib = pg._lib
    with open(os.path.join(ROOT, 'include', 'pggan_hip_kid.h')) as f:
        hdr = f.read()
    args, res, consts = _lib.parse_header(hdr)
    declared = set(re.findall(r'^int\s+(pg_\w+)\s*\(', hdr, flags=re.M))
    assert declared == set(args) == set(_lib.KID_SIGNATURES) == {'pg_kid_tilesums_f64'}
    P, I, L, D = _lib.P, _lib.I, _lib.L, _lib.D
    assert _lib.KID_SIGNATURES == {'pg_kid_tilesums_f64': [P, L, P, L, I, D, D, I, P, P]}
    assert all(r is I for r in res.values())
    assert consts == _lib.KID_CONSTANTS == {'PG_KID_TILE': 64, 'PG_KID_MIN_F': 16, 'PG_KID_MAX_F': 512}
    assert (pg.ops.KID_TILE, pg.ops.KID_MIN_F, pg.ops.KID_MAX_F) == (64, 16, 512)
    # additive: the product boundary is what it was, and no name is declared twice
    assert len(_lib.SIGNATURES) == 96 and _lib.ABI_VERSION == 27
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'KID_SIGNATURES']
    assert len(others) >= 15 and not any(set(_lib.KID_SIGNATURES) & set(t) for t in others)
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('CONSTANTS') and n != 'KID_CONSTANTS']
    assert not any(set(_lib.KID_CONSTANTS) & set(t) for t in others)


def test_library_exports_the_kid_symbol():
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    for name in pg._lib.KID_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.pg_abi_version() == pg._lib.ABI_VERSION
    assert pg.KernelDistance is M.KernelDistance and pg.kid_statistic is M.kid_statistic and pg.KIDMonitor is pg.plugins.KIDMonitor
    assert {'KernelDistance', 'kid_statistic', 'KIDMonitor'} <= set(pg.__all__)


# ---------------------------------------------------------------------------------------------------------------- the statistic
def _features(rows, F, seed, shift=0.0):
    return (np.random.RandomState(seed).randn(rows, F) * 0.5 + shift).astype(np.float32)


def _pairs(x, y):
    return (kid_ref.pairs_exact(x)[0], kid_ref.pairs_exact(y)[0], kid_ref.pairs_exact(x, y)[0])


def _tiles(kxx, kyy, kxy):
    off = lambda k: k - np.diag(np.diag(k))
    return kid_ref.tile_reduce(off(kxx)), kid_ref.tile_reduce(off(kyy)), kid_ref.tile_reduce(kxy)


def test_statistic_against_double_loops_ragged():
    """m, n = 130, 67.  The tile sums handed over are numpy sums of the pair values, the loops sum the same values exactly: on the path
    of any term lie at most 4095 additions of a tile sum (in whatever order numpy takes them), at most 8 of the statistic's sum over the
    tiles, a division and two additions -- fewer than TOL = 4112 roundings, each at most 2^-53 of the magnitudes' sum."""
    x, y = _features(130, 32, 1), _features(67, 32, 2, shift=0.1)
    kxx, kyy, kxy = _pairs(x, y)
    res = M.kid_statistic(*(_tiles(kxx, kyy, kxy) + (130, 67)))
    want, mag = kid_ref.kid_loops(kxx, kyy, kxy)
    print('ragged: kid %.12g, loops %.12g, error / bound = %.4f' % (res['kid'], want, abs(res['kid'] - want) / (TOL * kid_ref.U * mag)))
    assert abs(res['kid'] - want) <= TOL * kid_ref.U * mag
    assert (res['subsets'], res['kid_subset_mean'], res['kid_subset_std']) == (0, None, None)


def test_statistic_subsets_against_double_loops():
    """m = n = 200, subset_size 64: 3 subsets of rows [64 s, 64 s + 64) of both sets; the rows from 192 on are in no subset."""
    x, y = _features(200, 32, 3), _features(200, 32, 4, shift=0.05)
    kxx, kyy, kxy = _pairs(x, y)
    res = M.kid_statistic(*(_tiles(kxx, kyy, kxy) + (200, 200)), subset_size=64)
    want, mag = kid_ref.kid_loops(kxx, kyy, kxy)
    assert abs(res['kid'] - want) <= TOL * kid_ref.U * mag and res['subsets'] == 3
    per, mags = zip(*[kid_ref.kid_loops(kxx[b, b], kyy[b, b], kxy[b, b]) for b in (slice(64 * s, 64 * s + 64) for s in range(3))])
    mean, std = float(np.mean(per)), float(np.std(per, ddof=1))
    tol = TOL * kid_ref.U * max(mags)
    print('subsets: %s, mean %.6g, std %.6g' % (per, mean, std))
    assert abs(res['kid_subset_mean'] - mean) <= tol and abs(res['kid_subset_std'] - std) <= 4 * tol and std > 0
    one = M.kid_statistic(*(_tiles(kxx, kyy, kxy) + (200, 200)), subset_size=128)
    assert one['subsets'] == 1 and one['kid_subset_mean'] is None and one['kid_subset_std'] is None and one['kid'] == res['kid']
    assert M.kid_statistic(*(_tiles(kxx, kyy, kxy) + (200, 200)))['subsets'] == 0              # the default: subsets of 1024


def test_statistic_checks_its_arguments():
    s = np.zeros((3, 3))
    for args, kw in (((s, s, s, 130, 67), {}), ((s, s, s, 130, 130), {'subset_size': 100}), ((s, s, s, 130, 130), {'subset_size': 0}),
                     ((s, s, s, 1, 130), {}), ((s[:2, :2], s, s[:2], 128, 130), {'subset_size': 64.5})):
        with pytest.raises(ValueError):
            M.kid_statistic(*args, **kw)
    assert M.kid_statistic(s, s, s, 130, 130, subset_size=64)['kid'] == 0.0


def test_the_estimator_is_unbiased_where_the_frechet_distance_is_not():
    """200 draws of two sets of 64 vectors from the same N(0, I_128), rounded to float32: the true distance is 0.  The mean of kid lies
    within 3 standard errors of 0; the Frechet statistic of the same draws' moments is above 50 in every draw."""
    rs = np.random.RandomState(0)
    kid, fd = [], []
    for _ in range(200):
        x, y = rs.randn(64, 128).astype(np.float32), rs.randn(64, 128).astype(np.float32)
        sxx, syy, sxy = M._kid_tilesums_host(x, skip_diagonal=True), M._kid_tilesums_host(y, skip_diagonal=True), M._kid_tilesums_host(x, y)
        kid.append(M.kid_statistic(sxx, syy, sxy, 64, 64)['kid'])
        fd.append(M.frechet_statistic(*(M._moments_host(x) + M._moments_host(y)))['fd'])
    mean, se = float(np.mean(kid)), float(np.std(kid, ddof=1) / np.sqrt(200))
    print('kid over 200 draws: mean %.3e, standard error %.3e, ratio %.3f; fd %.1f .. %.1f, mean %.1f'
          % (mean, se, abs(mean) / se, min(fd), max(fd), float(np.mean(fd))))
    assert abs(mean) <= 3 * se
    assert min(fd) > 50


# ---------------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize('M_,N,F,skip', [(130, 67, 48, False), (130, 0, 16, True), (130, 0, 16, False), (1100, 70, 16, False)])
def test_host_tile_sums_within_the_summation_bound(M_, N, F, skip):
    """The twin is an fp64 evaluation in numpy's order: the any-order bound of tests/kid_ref.py holds for it as for the device.
    1100 rows: more than one of its blocks of 1024."""
    x = _features(M_, F, M_ + F, shift=0.2)
    y = _features(N, F, N + F) if N else None
    got = M._kid_tilesums_host(x, y, skip_diagonal=skip)
    want, bound = kid_ref.tilesums_exact(x, y, skip_diagonal=skip)
    print('host twin (%d, %d, %d): largest error / bound = %.4f' % (M_, N, F, (np.abs(got - want) / bound).max()))
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all()
    if not N:
        assert np.abs(got - got.T).max() <= bound.max()
    xi = np.random.RandomState(M_).randint(-3, 4, (M_, F)).astype(np.float32)
    assert np.array_equal(M._kid_tilesums_host(xi, None if not N else xi[:N], 1.0, 1.0, skip),
                          kid_ref.tilesums_int(xi, None if not N else xi[:N], 1, 1, skip).astype(np.float64))
    if N:
        with pytest.raises(ValueError):
            M._kid_tilesums_host(x, y, skip_diagonal=True)


def test_host_metric_end_to_end():
    reals, fakes = fd_ref.box_images(40, 1, 8, 2, seed=1), fd_ref.box_images(33, 1, 8, 1, seed=2)
    kd = M.KernelDistance(torch.from_numpy(reals), device='cpu', with_fd=True).fit()
    assert tuple(kd.features.shape) == (40, 128) and tuple(kd.sxx.shape) == (1, 1) and sorted(kd.indices.tolist()) == list(range(40))
    assert torch.equal(kd.indices, torch.randperm(40, generator=torch.Generator().manual_seed(0)))
    kd.feed_u8(torch.from_numpy(fakes[:20]))
    kd.feed(torch.from_numpy(fakes[20:].astype(np.float32) / 127.5 - 1))
    res = kd.result()
    assert set(res) == {'kid', 'subsets', 'kid_subset_mean', 'kid_subset_std', 'num_real', 'num_fake', 'fd', 'mean_term', 'cov_term'}
    fx, fy = kd.features.numpy(), kd.embedding(torch.from_numpy(fakes)).numpy()
    (sxx, bxx), (syy, byy), (sxy, bxy) = (kid_ref.tilesums_exact(fx, skip_diagonal=True), kid_ref.tilesums_exact(fy, skip_diagonal=True),
                                          kid_ref.tilesums_exact(fx, fy))
    want = M.kid_statistic(sxx, syy, sxy, 40, 33)['kid']
    assert abs(res['kid'] - want) <= kid_ref.kid_bound(bxx, byy, bxy, sxx, syy, sxy, 40, 33) and (res['num_real'], res['num_fake']) == (40, 33)
    fd = M.FrechetDistance(torch.from_numpy(reals), device='cpu').fit()
    fd.feed_u8(torch.from_numpy(fakes))
    assert res['fd'] == fd.result()['fd']
    with pytest.raises(RuntimeError):
        kd.feed_u8(torch.from_numpy(fakes))                                         # result() was taken
    kd.reset()
    kd.feed_u8(torch.from_numpy(reals)[kd.indices])
    kd.result()
    assert torch.equal(kd.syy, kd.sxx)
    few = M.KernelDistance(torch.from_numpy(reals), num_real=10, seed=3, gamma=0.5, coef0=0.0, device='cpu').fit()
    few.feed_u8(torch.from_numpy(fakes[:2]))
    k = (0.5 * few.features.double().numpy().dot(few.embedding(torch.from_numpy(fakes[:2])).double().numpy().T)) ** 3
    assert 'fd' not in few.result() and few.indices.numel() == 10 and abs(float(few.sxy.sum()) - k.sum()) <= 1e-12 * np.abs(k).sum()


def test_argument_errors():
    x = torch.from_numpy(fd_ref.box_images(6, 1, 8, 1, seed=1))
    for kw in ({'num_real': 1}, {'subset_size': 100}, {'subset_size': 0}, {'max_resolution': 24}, {'seed': 0.5},
               {'embedding': M.RandomEmbedding(1)}):
        with pytest.raises(ValueError):
            M.KernelDistance(x, device='cpu', **kw)
    with pytest.raises(ValueError):
        M.KernelDistance(x.float(), device='cpu')
    with pytest.raises(ValueError):
        M.KernelDistance(x, num_real=7, device='cpu').fit()
    m = M.KernelDistance(x, device='cpu')
    with pytest.raises(RuntimeError):
        m.feed_u8(x)                                                                 # fit() first
    with pytest.raises(RuntimeError):
        m.result()
    m.fit()
    with pytest.raises(ValueError):
        m.feed_u8(torch.zeros((2, 1, 16, 16), dtype=torch.uint8))                    # another shape
    m.feed_u8(x[:1])
    with pytest.raises(RuntimeError):
        m.result()                                                                   # one fake
    for call in (lambda: pg.ops.kid_tilesums_f64(torch.zeros(4, 16)), lambda: pg.ops.kid_tilesums_f64(None)):
        with pytest.raises(ValueError):
            call()                                                                   # host tensors: the wrapper takes device tensors only
    ds = types.SimpleNamespace()
    with pytest.raises(ValueError):
        pg.KIDMonitor(ds, None, num_samples=1)
    with pytest.raises(ValueError):
        pg.KIDMonitor(ds, None, minibatch=0)
    assert pg.KIDMonitor(ds, None, num_samples=2).num_samples == 2                   # no floor beyond 2


# ------------------------------------------------------------------------------------------------------------------ monitor
class _Latents(object):
    """What ``sample_fn`` returns on a host without a device: ``.cuda()`` hands the tensor on."""

    def __init__(self, z):
        self.z = z

    def cuda(self):
        return self.z


class _StubG(object):
    """'Generates' training images of the data set's current stage, picked by the latent's first column, plus a constant."""

    def __init__(self, ds, shift):
        self.ds, self.shift, self.calls = ds, shift, 0

    def forward(self, z):
        self.calls += 1
        level = self.ds.level_stack().float()
        idx = (z[:, 0].abs() * 1000).long() % level.shape[0]
        return ((level[idx] + self.shift).clamp(0, 255) / 127.5 - 1).contiguous()


def test_monitor_on_the_twin_refits_on_a_stage_change_and_writes_the_spread():
    stack = fd_ref.box_images(140, 1, 16, 2, seed=8)
    ds = pg.DeviceImageDataset(stack, model_initial_depth=1, device='cpu')      # 8x8
    G, Gs = _StubG(ds, 0.0), _StubG(ds, 40.0)
    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=0, G=G, g_ema=types.SimpleNamespace(network=lambda: Gs))
    g = torch.Generator().manual_seed(2)
    drawn = []

    def sample_fn(n):
        drawn.append(n)
        return _Latents(torch.randn(n, 4, generator=g))

    mon = pg.KIDMonitor(ds, sample_fn, num_samples=130, minibatch=64, kid_ticks=1, subset_size=64, device='cpu')
    assert mon.trigger_interval == [(1, 'epoch'), (1, 'end')]
    mon.register(trainer)
    mon.epoch(1)
    st = trainer.stats
    assert set(st) == {'kid', 'kid_std'} and drawn == [64, 64, 2] and (G.calls, Gs.calls) == (0, 3)
    metric = mon._metric_obj
    res = metric.result()
    assert metric.resolution == 8 and res['subsets'] == 2 and (res['num_real'], res['num_fake']) == (140, 130)
    assert st['kid']['val'] == res['kid'] and st['kid_std']['val'] == res['kid_subset_std'] and res['kid'] > 0
    first = metric.sxx
    mon.epoch(2)                                                                 # the same stage: no refit
    assert mon._metric_obj is metric and metric.sxx is first
    ds.model_depth = 2                                                           # 16x16
    mon.end(3)
    assert metric.resolution == 16 and metric.shape == (1, 16, 16) and metric.sxx is not first
    both = pg.KIDMonitor(ds, sample_fn, num_samples=8, minibatch=8, smoothed=False, num_real=30, with_fd=True, device='cpu')
    both.register(trainer)
    trainer.stats.clear()
    both.epoch(1)
    assert set(trainer.stats) == {'kid', 'fd'} and G.calls == 1 and both._metric_obj.indices.numel() == 30
    other = types.SimpleNamespace(stats={}, parallel=types.SimpleNamespace(rank=1), G=G, g_ema=None)
    both.register(other)
    both.epoch(1)
    assert other.stats == {}                                                     # rank 0 evaluates
