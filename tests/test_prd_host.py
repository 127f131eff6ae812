"""metrics.PrecisionRecall's numpy twin (device='cpu') against tests/prd_ref.py, the binding of include/pggan_hip_prd.h, and
plugins.PRDMonitor on the twin with a stub trainer.  Integer arithmetic: every comparison is ``==``.  Host tests: no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import prd_ref
from dataset_ref import make_stack

import pggan_amd as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX = np.iinfo(np.int64).max


def rows(x):
    return x.reshape(len(x), -1)


def same_counts(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == np.int32 and g.tolist() == w


# ------------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize('C,r,Na,Nb,k', [(1, 4, 9, 7, 1), (3, 4, 33, 20, 3), (3, 8, 20, 40, 16)])
def test_twin_equals_the_reference_on_random_sets(C, r, Na, Nb, k):
    a, b = prd_ref.images(Na, C, r, seed=7 * r + C), prd_ref.images(Nb, C, r, seed=7 * r + C + 2)
    rad_a, rad_b = pg.metrics._radii_host(rows(a), k), pg.metrics._radii_host(rows(b), k)
    assert rad_a.dtype == np.int64 and rad_a.tolist() == prd_ref.radii(a, k).tolist() and rad_b.tolist() == prd_ref.radii(b, k).tolist()
    for ra, rb in ((rad_a, rad_b), (rad_a, None), (None, rad_b)):
        same_counts(pg.metrics._ball_host(rows(a), rows(b), ra, rb), prd_ref.ball_counts(a, b, ra, rb))


@pytest.mark.parametrize('k', [1, 3, 5])
def test_metric_on_the_twin_equals_the_reference(k):
    reals, fakes = prd_ref.images(50, 3, 4, seed=1), prd_ref.images(37, 3, 4, seed=2)
    fakes[:9] = np.clip(reals[:9].astype(np.int32) + 3, 0, 255).astype(np.uint8)       # some fakes near reals: not every count is 0
    m = pg.metrics.PrecisionRecall(torch.from_numpy(reals), k=k, device='cpu').fit()
    assert m.radii.dtype == torch.int64 and sorted(m.indices.tolist()) == list(range(50)) and m.resolution == 4
    for batch in (37, 16, 1):
        m.reset()
        for s in range(0, 37, batch):
            m.feed_u8(torch.from_numpy(fakes[s:s + batch]))
        res = m.result()
        want = prd_ref.prd(reals[m.indices.numpy()], fakes, k)
        assert {n: res[n] for n in want} == want and (res['num_real'], res['num_fake'], res['k']) == (50, 37, k)
        assert 0 < res['precision'] <= 1 and 0 < res['coverage'] < 1
    as_fp32 = torch.from_numpy(fakes.astype(np.float32) / 127.5 - 1)
    m.reset()
    m.feed(as_fp32)
    assert m.result() == res
    with pytest.raises(RuntimeError):
        m.feed(as_fp32)                                                      # result() was taken


def test_num_real_takes_a_seeded_subset():
    stack = prd_ref.images(60, 1, 4, seed=3)
    fakes = prd_ref.images(12, 1, 4, seed=4)
    m = pg.metrics.PrecisionRecall(torch.from_numpy(stack), k=2, num_real=25, seed=5, device='cpu').fit()
    idx = m.indices.tolist()
    assert idx == torch.randperm(60, generator=torch.Generator().manual_seed(5))[:25].tolist() and len(set(idx)) == 25
    assert np.array_equal(m.reals.numpy(), stack[idx]) and m.radii.tolist() == prd_ref.radii(stack[idx], 2).tolist()
    m.feed_u8(torch.from_numpy(fakes))
    want = prd_ref.prd(stack[idx], fakes, 2)
    assert {n: m.result()[n] for n in want} == want and m.result()['num_real'] == 25


def test_identical_sets():
    """R = G with all distances distinct: every ball holds its own centre and its k nearest, so precision = recall = coverage = 1 and
    density = (k + 1) / k exactly."""
    x = prd_ref.images(40, 3, 8, seed=9)
    d = prd_ref.d2(x, x)
    assert len(set(d[np.triu_indices(40, 1)].tolist())) == 40 * 39 // 2
    for k in (1, 3, 7):
        m = pg.metrics.PrecisionRecall(torch.from_numpy(x), k=k, device='cpu').fit()
        m.feed_u8(torch.from_numpy(x))
        res = m.result()
        assert (res['precision'], res['recall'], res['coverage']) == (1.0, 1.0, 1.0) and res['density'] == (k + 1) / float(k)
        assert prd_ref.prd(x, x, k)['density'] == (k + 1) / float(k)


def test_two_clusters():
    reals, fakes = prd_ref.two_clusters()
    k = 3
    rad_r, rad_f = pg.metrics._radii_host(rows(reals), k), pg.metrics._radii_host(rows(fakes), k)
    assert rad_r.max() <= 63 * 63 * 192 and rad_f.max() <= 63 * 63 * 192 < 129 * 129 * 192 <= prd_ref.d2(reals[40:], fakes).min()
    a_cnt, a_hit, b_cnt, b_hit = pg.metrics._ball_host(rows(fakes), rows(reals), rad_f, rad_r)
    same_counts((a_cnt, a_hit, b_cnt, b_hit), prd_ref.ball_counts(fakes, reals, rad_f, rad_r))
    assert b_cnt[40:].tolist() == [0] * 24 and b_hit[40:].tolist() == [0] * 24
    m = pg.metrics.PrecisionRecall(torch.from_numpy(reals), k=k, device='cpu').fit()
    m.feed_u8(torch.from_numpy(fakes))
    res = m.result()
    assert res['recall'] <= 40 / 64.0 and res['coverage'] <= 40 / 64.0
    want = prd_ref.prd(reals[m.indices.numpy()], fakes, k)
    assert {n: res[n] for n in want} == want


def test_a_duplicate_at_another_index_gives_radius_zero():
    x = prd_ref.images(12, 1, 4, seed=11)
    x[7] = x[2]
    rad = pg.metrics._radii_host(rows(x), 1)
    assert rad[2] == rad[7] == 0 and (np.delete(rad, [2, 7]) > 0).all() and rad.tolist() == prd_ref.radii(x, 1).tolist()
    assert pg.metrics._radii_host(rows(x), 2)[2] > 0                         # the exclusion is by index: one duplicate, one zero


def test_the_boundary_is_inside():
    a, b = prd_ref.images(6, 1, 4, seed=12), prd_ref.images(5, 1, 4, seed=13)
    d = prd_ref.d2(a, b)
    rad_b = d[1].copy()                                                      # probe 1 sits ON every ball of b
    rad_a = d[:, 3].copy()                                                   # centre 3 sits ON every ball of a
    a_cnt, a_hit, b_cnt, b_hit = pg.metrics._ball_host(rows(a), rows(b), rad_a, rad_b)
    assert a_cnt[1] == 5 and (b_hit >= 1).all() and b_cnt[3] == 6 and (a_hit >= 1).all()
    same_counts((a_cnt, a_hit, b_cnt, b_hit), prd_ref.ball_counts(a, b, rad_a, rad_b))
    below = pg.metrics._ball_host(rows(a), rows(b), rad_a - 1, rad_b - 1)
    same_counts(below, prd_ref.ball_counts(a, b, rad_a - 1, rad_b - 1))
    assert below[0][1] < 5 and below[2][3] < 6


def test_argument_errors():
    x = torch.from_numpy(prd_ref.images(8, 1, 4, seed=14))
    for k in (0, 17, True, 1.5):
        with pytest.raises(ValueError):
            pg.metrics.PrecisionRecall(x, k=k, device='cpu')
    with pytest.raises(ValueError):
        pg.metrics.PrecisionRecall(x, k=8, device='cpu').fit()               # N <= k
    with pytest.raises(ValueError):
        pg.metrics.PrecisionRecall(x, k=3, num_real=3, device='cpu')         # num_real <= k
    with pytest.raises(ValueError):
        pg.metrics.PrecisionRecall(x, k=3, num_real=9, device='cpu').fit()   # more than there are
    with pytest.raises(ValueError):
        pg.metrics.PrecisionRecall(torch.zeros((8, 1, 2, 2), dtype=torch.uint8), k=3, device='cpu').fit()     # D = 4
    with pytest.raises(ValueError):
        pg.metrics.PrecisionRecall(x.float(), k=3, device='cpu')
    with pytest.raises(ValueError):
        pg.metrics.PrecisionRecall(x, k=3, max_resolution=3, device='cpu')
    with pytest.raises(ValueError):
        pg.metrics.PrecisionRecall(x, k=3, drange=(1, 1), device='cpu')
    m = pg.metrics.PrecisionRecall(x, k=3, device='cpu')
    with pytest.raises(RuntimeError):
        m.feed_u8(x)                                                         # fit() first
    m.fit()
    with pytest.raises(ValueError):
        m.feed_u8(torch.zeros((2, 1, 8, 8), dtype=torch.uint8))              # another shape
    with pytest.raises(ValueError):
        m.feed_u8(x.float())
    with pytest.raises(ValueError):
        m.feed(x)
    m.feed_u8(x[:3])
    with pytest.raises(RuntimeError):
        m.result()                                                           # 3 fakes for k = 3
    for call in (lambda: pg.ops.prd_kth_u8(x, 3), lambda: pg.ops.prd_ball_u8(x, x, None, torch.zeros(8, dtype=torch.int64))):
        with pytest.raises(ValueError):
            call()                                                           # host tensors: the wrappers take device tensors only


def test_max_resolution_reduces_both_sets():
    stack = make_stack(30, 3, 16, seed=2)
    fakes = make_stack(10, 3, 16, seed=3)
    m = pg.metrics.PrecisionRecall(torch.from_numpy(stack), k=2, max_resolution=4, device='cpu').fit()
    assert tuple(m.reals.shape) == (30, 3, 4, 4) and m.resolution == 16
    low = pg.dataset.level_host(stack, 2)
    assert np.array_equal(m.reals.numpy(), low[m.indices.numpy()])
    m.feed_u8(torch.from_numpy(fakes))
    want = prd_ref.prd(low[m.indices.numpy()], pg.dataset.level_host(fakes, 2), 2)
    assert {n: m.result()[n] for n in want} == want
    same = pg.metrics.PrecisionRecall(torch.from_numpy(stack), k=2, max_resolution=32, device='cpu').fit()
    assert tuple(same.reals.shape) == (30, 3, 16, 16)


# ------------------------------------------------------------------------------------------------------------------ binding
def test_prd_header_is_derived_completely_and_the_product_tables_are_unchanged():
    _lib = pg._lib
    with open(os.path.join(ROOT, 'include', 'pggan_hip_prd.h')) as f:
        hdr = f.read()
    args, res, consts = _lib.parse_header(hdr)
    declared = set(re.findall(r'^int\s+(pg_\w+)\s*\(', hdr, flags=re.M))
    assert declared == set(args) == set(_lib.PRD_SIGNATURES) == {'pg_prd_kth_u8', 'pg_prd_ball_u8'}
    P, I, L = _lib.P, _lib.I, _lib.L
    assert _lib.PRD_SIGNATURES == {'pg_prd_kth_u8': [P, L, L, I, P, P], 'pg_prd_ball_u8': [P, L, P, L, L, P, P, P, P, P, P, P]}
    assert all(r is I for r in res.values())
    assert consts == _lib.PRD_CONSTANTS == {'PG_PRD_TILE': 128} and pg.ops.PRD_TILE == 128
    # additive: the product boundary is what it was
    assert len(_lib.SIGNATURES) == 96 and _lib.ABI_VERSION == 27
    assert not set(_lib.PRD_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.DEBUG_SIGNATURES))
    assert not set(_lib.PRD_CONSTANTS) & set(_lib.CONSTANTS)


def test_library_exports_the_prd_symbols():
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    for name in pg._lib.PRD_SIGNATURES:
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
    drawn, latents = [], []

    def sample_fn(n):
        drawn.append(n)
        latents.append(torch.randn(n, 4, generator=g))
        return _Latents(latents[-1])

    mon = pg.PRDMonitor(ds, sample_fn, num_samples=40, minibatch=16, k=2, prd_ticks=1, device='cpu')
    assert mon.trigger_interval == [(1, 'epoch'), (1, 'end')]
    mon.register(trainer)
    mon.epoch(1)
    st = trainer.stats
    assert set(st) == {'precision', 'recall', 'density', 'coverage'} and drawn == [16, 16, 8] and (G.calls, Gs.calls) == (0, 3)
    metric = mon._metric_obj
    assert metric.resolution == 8 and metric.k == 2 and tuple(metric.reals.shape) == (60, 1, 8, 8)
    res = metric.result()
    assert all(st[n]['val'] == res[n] for n in st) and res['num_fake'] == 40
    fakes = pg.metrics._quantise_host(torch.cat([_StubG(ds, 40.0).forward(z) for z in latents]).numpy(), (-1, 1))
    want = prd_ref.prd(ds.level_stack().numpy()[metric.indices.numpy()], fakes, 2)
    assert {n: res[n] for n in want} == want
    first = metric.radii.clone()
    mon.epoch(2)                                                                 # the same stage: no refit
    assert mon._metric_obj is metric and torch.equal(metric.radii, first)
    ds.model_depth = 2                                                           # 16x16
    mon.end(3)
    assert metric.resolution == 16 and tuple(metric.reals.shape) == (60, 1, 16, 16)
    assert metric.radii.tolist() == prd_ref.radii(stack[metric.indices.numpy()], 2).tolist()
    raw = pg.PRDMonitor(ds, sample_fn, num_samples=8, minibatch=8, k=1, smoothed=False, max_resolution=8, device='cpu')
    raw.register(trainer)
    raw.epoch(1)
    assert G.calls == 1 and tuple(raw._metric_obj.reals.shape) == (60, 1, 8, 8) and trainer.stats['precision']['val'] == 1.0
    with pytest.raises(ValueError):
        pg.PRDMonitor(ds, sample_fn, smoothed=True, device='cpu').register(types.SimpleNamespace(g_ema=None))
    with pytest.raises(ValueError):
        pg.PRDMonitor(ds, sample_fn, num_samples=3, k=3)
    other = types.SimpleNamespace(stats={}, parallel=types.SimpleNamespace(rank=1), G=G, g_ema=None)
    raw.register(other)
    raw.epoch(1)
    assert other.stats == {}                                                     # rank 0 evaluates
    assert pg.PRDMonitor(ds, sample_fn).precision == 'fp32' and pg.PRDMonitor(ds, sample_fn, precision='bf16').precision == 'bf16'
