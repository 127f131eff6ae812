"""metrics.NDB's numpy twin (device='cpu') against tests/ndb_ref.py, the binding of include/pggan_hip_cluster.h, and plugins.NDBMonitor
on the twin with a stub trainer.  Integer arithmetic: every comparison is ``==``.  Host tests: no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ndb_ref
from dataset_ref import make_stack

import pggan_amd as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (blobs, images per blob, C, r, K, holdout): the two planted cases of the issue
PLANTED = [(6, 40, 1, 16, 6, 0), (10, 24, 3, 8, 16, 48)]


def planted(blobs, per_blob, C, r, seed=3):
    return ndb_ref.planted_images(ndb_ref.planted_centres(blobs, C, r, seed), per_blob, seed + 1)


_fits = {}


def ref_fit(case, seed=0, max_iter=30):
    """The reference's fit of a planted case, made once and shared."""
    key = (case, seed, max_iter)
    if key not in _fits:
        blobs, per_blob, C, r, K, h = case
        x = planted(blobs, per_blob, C, r)
        _fits[key] = (x, ndb_ref.fit(x, K, h, seed, max_iter))
    return _fits[key]


def same_fit(ndb, want):
    assert np.array_equal(ndb.labels.cpu().numpy(), np.array(want['labels'], dtype=np.int32)) and ndb.labels.dtype == torch.int32
    assert np.array_equal(ndb.centroids.cpu().numpy(), want['centroids']) and ndb.centroids.dtype == torch.uint8
    assert ndb.ref.tolist() == want['ref'] and ndb.ref.dtype == np.int64
    assert (ndb.iterations, ndb.converged) == (want['iterations'], want['converged'])


@pytest.mark.parametrize('case', PLANTED)
def test_twin_equals_the_reference_on_planted_clusters(case):
    blobs, per_blob, C, r, K, h = case
    x, want = ref_fit(case)
    ndb = pg.metrics.NDB(torch.from_numpy(x), k=K, holdout=h, device='cpu').fit()
    same_fit(ndb, want)
    assert want['converged'] and 2 <= want['iterations'] < 30 and ndb.resolution == r
    assert sum(want['ref']) == (h if h else x.shape[0])
    fresh = ndb_ref.planted_images(ndb_ref.planted_centres(blobs, C, r, 3), 20, 77)
    gen = ndb_ref.histogram(fresh, want['centroids'])
    for batch in (1, 16, 64):                                                    # any split of the samples, the same histogram
        ndb.reset()
        for a in range(0, fresh.shape[0], batch):
            ndb.feed_u8(torch.from_numpy(fresh[a:a + batch]))
        res = ndb.result()
        assert res['gen'].tolist() == gen and res['ref'].tolist() == want['ref'] and res['num_samples'] == fresh.shape[0]
    stat = ndb_ref.statistic(want['ref'], gen)
    assert res['ndb'] == stat['ndb'] and res['ndb_over_k'] == stat['ndb_over_k'] and res['k'] == K
    assert np.array_equal(res['z'], np.array(stat['z'])) and res['jsd'] == stat['jsd']
    # fp32 samples go through the saved image's rounding
    ndb.reset()
    ndb.feed(torch.from_numpy(fresh.astype(np.float32) / 127.5 - 1))
    assert ndb.result()['gen'].tolist() == gen
    with pytest.raises(RuntimeError):
        ndb.feed_u8(torch.from_numpy(fresh[:1]))                                 # result() was taken
    with pytest.raises(ValueError):
        ndb.reset() or ndb.feed_u8(torch.zeros((2, C, 2 * r, 2 * r), dtype=torch.uint8))        # another resolution than the fitted one


def test_duplicate_initial_centroids_the_lower_wins_and_the_empty_bin_keeps_its_centroid():
    blobs, per_blob, C, r, K, h = PLANTED[0]
    x = planted(blobs, per_blob, C, r).copy()
    _, fitset = ndb_ref.split(x.shape[0], 0, 5)
    init = ndb_ref.initial(fitset, K, 5)
    lo, hi = 1, 4
    x[init[hi]] = x[init[lo]]                                                    # bins 1 and 4 start on equal images
    first, _ = ndb_ref.assign(x, x[init])
    assert hi not in first and first[init[hi]] == lo and first[init[lo]] == lo
    want = ndb_ref.fit(x, K, 0, 5, max_iter=1)
    assert np.array_equal(want['centroids'][hi], x[init[hi]]) and not want['converged'] and want['iterations'] == 1
    assert not np.array_equal(want['centroids'][lo], x[init[lo]])                # the bin with members moved
    same_fit(pg.metrics.NDB(torch.from_numpy(x), k=K, seed=5, max_iter=1, device='cpu').fit(), want)
    same_fit(pg.metrics.NDB(torch.from_numpy(x), k=K, seed=5, device='cpu').fit(), ndb_ref.fit(x, K, 0, 5))


def test_max_iter_is_a_condition():
    x, want = ref_fit(PLANTED[0], max_iter=1)
    assert want['iterations'] == 1 and not want['converged']
    ndb = pg.metrics.NDB(torch.from_numpy(x), k=PLANTED[0][4], max_iter=1, device='cpu').fit()
    same_fit(ndb, want)
    # the labels are the assignment to the FINAL centroids
    assert ndb.labels.tolist() == ndb_ref.assign(x, want['centroids'])[0]


def test_holdout_bounds_and_disjoint_split():
    x = torch.from_numpy(planted(4, 5, 1, 4))                                    # M = 20
    for bad in (-1, 20 - 6 + 1, 20, True, 2.5):
        with pytest.raises(ValueError):
            pg.metrics.NDB(x, k=6, holdout=bad, device='cpu')
    for bad_k in (1, pg.ops.NN_MAX_QUERIES + 1, True):
        with pytest.raises(ValueError):
            pg.metrics.NDB(x, k=bad_k, device='cpu')
    with pytest.raises(ValueError):
        pg.metrics.NDB(x.float(), k=2, device='cpu')
    ndb = pg.metrics.NDB(x, k=6, holdout=14, seed=9, device='cpu')               # the largest: the fit set is exactly k images
    held, fit = ndb.split()
    assert held.tolist() == ndb_ref.split(20, 14, 9)[0] and fit.tolist() == ndb_ref.split(20, 14, 9)[1]
    assert len(held) == 14 and len(fit) == 6 and sorted(held.tolist() + fit.tolist()) == list(range(20))
    ndb.fit()
    same_fit(ndb, ndb_ref.fit(x.numpy(), 6, 14, 9))
    assert int(ndb.ref.sum()) == 14
    with pytest.raises(RuntimeError):
        ndb.result()                                                             # nothing was fed
    with pytest.raises(RuntimeError):
        pg.metrics.NDB(x, k=6, device='cpu').feed_u8(x)                          # not fitted


def test_a_holdout_reference_tells_dropped_modes_from_a_fresh_sample():
    """8 blobs of 200 images of 1x32x32, K = 50, 400 held out: a fresh sample of the same distribution differs in few bins, one with two
    blobs dropped in many.  Asserted against the reference's own values, and the strict inequality between them."""
    centres = ndb_ref.planted_centres(8, 1, 32, 11)
    x = ndb_ref.planted_images(centres, 200, 12)
    same = ndb_ref.planted_images(centres, 100, 13)
    dropped = ndb_ref.planted_images(centres, 100, 13, drop=(2, 5))
    ndb = pg.metrics.NDB(torch.from_numpy(x), k=50, holdout=400, device='cpu').fit()
    c = ndb.centroids.numpy()
    want = {}
    for name, sample in (('same', same), ('dropped', dropped)):
        ndb.reset()
        ndb.feed_u8(torch.from_numpy(sample))
        res = ndb.result()
        gen = ndb_ref.histogram(sample, c)
        want[name] = ndb_ref.statistic(ndb.ref.tolist(), gen)
        assert res['gen'].tolist() == gen and res['ndb'] == want[name]['ndb']
    assert want['same']['ndb'] < want['dropped']['ndb'] and want['same']['jsd'] < want['dropped']['jsd']


# ------------------------------------------------------------------------------------------------------------------ binding
def test_cluster_header_is_derived_completely_and_the_product_tables_are_unchanged():
    _lib = pg._lib
    with open(os.path.join(ROOT, 'include', 'pggan_hip_cluster.h')) as f:
        hdr = f.read()
    args, res, consts = _lib.parse_header(hdr)
    declared = set(re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', hdr))
    assert declared == set(args) == set(_lib.CLUSTER_SIGNATURES) == {'pg_cluster_argmin_i64', 'pg_cluster_sums_u8', 'pg_cluster_centroids_u8'}
    P, I, L = _lib.P, _lib.I, _lib.L
    assert _lib.CLUSTER_SIGNATURES == {'pg_cluster_argmin_i64': [P, I, L, P, P, P], 'pg_cluster_sums_u8': [P, L, L, P, L, P, I, P, P],
                                       'pg_cluster_centroids_u8': [P, P, P, I, L, P]}
    assert all(r is I for r in res.values())
    assert consts == _lib.CLUSTER_CONSTANTS == {'PG_CLUSTER_MAX_IMAGES': 1 << 23} and pg.cluster.MAX_IMAGES == 1 << 23
    assert 255 * pg.cluster.MAX_IMAGES < 2 ** 31 <= 255 * (pg.cluster.MAX_IMAGES + 2 ** 16)
    # additive: the product boundary is what it was
    assert len(_lib.SIGNATURES) == 96 and len(_lib.CONSTANTS) == 27 and _lib.ABI_VERSION == 27
    assert not set(_lib.CLUSTER_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.DEBUG_SIGNATURES))
    assert not set(_lib.CLUSTER_CONSTANTS) & set(_lib.CONSTANTS)
    assert pg.cluster.MAX_BINS == _lib.CONSTANTS['PG_NN_MAX_QUERIES']


def test_library_exports_the_cluster_symbols():
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    for name in pg._lib.CLUSTER_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.pg_abi_version() == pg._lib.ABI_VERSION


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


def test_monitor_on_the_twin_refits_on_a_stage_change_and_respects_smoothed():
    stack = make_stack(60, 1, 16, seed=8)
    ds = pg.DeviceImageDataset(stack, model_initial_depth=1, device='cpu')      # 8x8
    G, Gs = _StubG(ds, 0.0), _StubG(ds, 40.0)
    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=0, G=G, g_ema=types.SimpleNamespace(network=lambda: Gs))
    g = torch.Generator().manual_seed(2)
    drawn = []

    def sample_fn(n):
        drawn.append(n)
        return _Latents(torch.randn(n, 4, generator=g))

    mon = pg.NDBMonitor(ds, sample_fn, num_samples=40, minibatch=16, k=5, ndb_ticks=1, device='cpu')
    assert mon.holdout == 12 and mon.trigger_interval == [(1, 'epoch'), (1, 'end')]
    mon.register(trainer)
    mon.epoch(1)
    st = trainer.stats
    assert set(st) == {'ndb', 'ndb_over_k', 'jsd'} and drawn == [16, 16, 8] and (G.calls, Gs.calls) == (0, 3)      # smoothed=None: Gs
    metric = mon._metric_obj
    assert metric.resolution == 8 and metric.holdout == 12 and metric.k == 5
    res = metric.result()
    assert (st['ndb']['val'], st['ndb_over_k']['val'], st['jsd']['val']) == (res['ndb'], res['ndb'] / 5.0, res['jsd'])
    assert int(res['gen'].sum()) == 40 and 0.0 <= res['jsd'] <= 1.0
    same_fit(metric, ndb_ref.fit(ds.level_stack().numpy(), 5, 12, 0))
    first_centroids = metric.centroids.clone()
    mon.epoch(2)                                                                 # the same stage: no refit
    assert mon._metric_obj is metric and torch.equal(metric.centroids, first_centroids)
    ds.model_depth = 2                                                           # 16x16
    mon.end(3)
    assert metric.resolution == 16 and tuple(metric.centroids.shape) == (5, 1, 16, 16)
    same_fit(metric, ndb_ref.fit(stack, 5, 12, 0))
    raw = pg.NDBMonitor(ds, sample_fn, num_samples=8, minibatch=8, k=5, holdout=0, smoothed=False, device='cpu')
    raw.register(trainer)
    raw.epoch(1)
    assert G.calls == 1 and raw._metric_obj.holdout == 0
    with pytest.raises(ValueError):
        pg.NDBMonitor(ds, sample_fn, smoothed=True, device='cpu').register(types.SimpleNamespace(g_ema=None))
    other = types.SimpleNamespace(stats={}, parallel=types.SimpleNamespace(rank=1), G=G, g_ema=None)
    raw.register(other)
    raw.epoch(1)
    assert other.stats == {}                                                     # rank 0 evaluates
