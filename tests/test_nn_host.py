"""Host side of the nearest-neighbour search: ``metrics.NearestNeighbours(device='cpu')`` (the numpy twin of the device path) against
tests/nn_ref.py, ``DeviceImageDataset.level_stack`` in host mode, ``plugins.NNMonitor`` over a host-mode data set with a stub trainer
(nothing touches a device: the monitor then runs the twin), and the argument errors that need no device.  The kernels are checked on
the device (tests/test_nn_gpu.py).  Every comparison is exact."""
import numpy as np
import pytest
import torch

import nn_ref
from dataset_ref import make_stack

import pggan_amd as pg


def _as_samples(images_u8, drange=(-1, 1)):
    """fp32 images in ``drange`` whose 0..255 levels are exactly ``images_u8`` (the data set's own range change)."""
    return torch.from_numpy(pg.dataset.prepare_host(images_u8, 1.0, (0, 255), drange))


def _result_arrays(res):
    return tuple(res[name].numpy() for name in ('sqdist', 'index', 'mirrored'))


def test_names_and_signatures():
    P, I, L, F = pg._lib.P, pg._lib.I, pg._lib.L, pg._lib.F
    assert pg._lib.SIGNATURES['pg_quantize_u8'] == [P, P, L, F, F, P]
    assert pg._lib.SIGNATURES['pg_l2dist_u8'] == [P, L, P, I, L, P, P]
    assert pg._lib.SIGNATURES['pg_topk_smallest_i64'] == [P, I, L, I, P, P, P]
    assert pg._lib.ABI_VERSION == 27                                         # additive: the version stays
    assert pg.NNMonitor is pg.plugins.NNMonitor and pg.NearestNeighbours is pg.metrics.NearestNeighbours
    assert 'NNMonitor' in pg.__all__ and 'NearestNeighbours' in pg.__all__
    assert pg.ops.NN_MAX_QUERIES >= 1 and pg.ops.NN_MAX_TOPK == 16
    for name in ('quantize_u8', 'l2dist_u8', 'topk_smallest_i64', 'nn_search_u8'):
        assert callable(getattr(pg.ops, name))


@pytest.mark.parametrize('C,r', [(1, 4), (3, 4), (3, 8)])
@pytest.mark.parametrize('mirror', [False, True])
def test_host_search_equals_the_reference(C, r, mirror):
    M, K, k = 37, 9, 5
    stack = nn_ref.images(M, C, r, seed=3)
    queries = nn_ref.images(K, C, r, seed=4)
    queries[2] = stack[11]                                                   # a copy ...
    queries[3] = stack[20][..., ::-1]                                        # ... and a mirrored copy
    stack[30] = stack[11]                                                    # a duplicate in the stack: the lower index comes first
    nn = pg.metrics.NearestNeighbours(torch.from_numpy(stack), k=k, mirror=mirror, device='cpu')
    res = nn.search(_as_samples(queries))
    sq, ix, mr = _result_arrays(res)
    if mirror:
        want = nn_ref.search_mirror(stack, queries, k)
    else:
        want = nn_ref.search(stack, queries, k) + (np.zeros((K, k), dtype=bool),)
    assert np.array_equal(sq, want[0]) and np.array_equal(ix, want[1]) and np.array_equal(mr, want[2])
    assert sq.dtype == np.int64 and ix.dtype == np.int64 and mr.dtype == bool and sq.shape == (K, k)
    assert res['rms'].dtype == torch.float64 and np.array_equal(res['rms'].numpy(), np.sqrt(want[0].astype(np.float64) / (C * r * r)))
    assert (sq[2, 0], ix[2, 0], sq[2, 1], ix[2, 1]) == (0, 11, 0, 30)
    if mirror:
        assert (sq[3, 0], ix[3, 0], bool(mr[3, 0])) == (0, 20, True)
    else:
        assert sq[3, 0] > 0
    # the images the result names, mirrored where it says so
    near = nn.neighbours(res)
    assert near.dtype == torch.float32 and tuple(near.shape) == (K, k, C, r, r)
    want_img = pg.dataset.batch_host(stack, ix.reshape(-1), mr.reshape(-1).astype(np.uint8), 0, 1.0, (0, 255), (-1, 1))
    assert np.array_equal(near.numpy().reshape(want_img.shape), want_img)


def test_host_search_with_k_equal_to_M_and_a_symmetric_image():
    M, C, r = 6, 1, 4
    stack = nn_ref.images(M, C, r, seed=8)
    stack[4] = np.concatenate([stack[4][..., :2], stack[4][..., 1::-1]], axis=-1)       # its own mirror image
    queries = stack[[4, 1]]
    for mirror in (False, True):
        res = pg.metrics.NearestNeighbours(torch.from_numpy(stack), k=M, mirror=mirror, device='cpu').search(_as_samples(queries))
        sq, ix, mr = _result_arrays(res)
        if mirror:
            want = nn_ref.search_mirror(stack, queries, M)
            assert (sq[0, 0], ix[0, 0], mr[0, 0], sq[0, 1], ix[0, 1], mr[0, 1]) == (0, 4, False, 0, 4, True)   # (sqdist, index, mirrored)
        else:
            want = nn_ref.search(stack, queries, M) + (np.zeros((2, M), dtype=bool),)
            assert sorted(ix[0]) == list(range(M))
        assert np.array_equal(sq, want[0]) and np.array_equal(ix, want[1]) and np.array_equal(mr, want[2])


def test_host_quantisation_is_the_saved_image():
    import msssim_ref
    x = torch.tensor([-1.2, -1.0, -0.99607843, 0.0, 0.00392157, 0.5, 1.0, 1.7, (2.5 / 127.5) - 1, (3.5 / 127.5) - 1], dtype=torch.float32)
    for drange in ((-1, 1), (0, 1), (-2.5, 3.0)):
        got = pg.metrics._quantise_host(x.numpy(), drange)
        assert np.array_equal(got, msssim_ref.quantise(x, drange).numpy().astype(np.uint8))


@pytest.mark.parametrize('pyramid', ['chain', 'direct'])
def test_level_stack_in_host_mode(pyramid):
    stack = make_stack(5, 3, 16, seed=6)
    ds = pg.DeviceImageDataset(stack, pyramid=pyramid, device='cpu')
    for model_depth, r in ((2, 16), (1, 8), (0, 4)):
        ds.model_depth = model_depth
        level = ds.level_stack()
        assert level.dtype == torch.uint8 and tuple(level.shape) == (5, 3, r, r) and level.is_contiguous()
        if pyramid == 'chain':
            want = stack
            for _ in range(2 - model_depth):
                want = pg.dataset.level_host(want, 1)
            assert level.data_ptr() == ds._levels[model_depth + 2].data_ptr()            # the stored level, no copy
        else:
            want = pg.dataset.level_host(stack, 2 - model_depth)
            assert (level.data_ptr() == ds._levels[4].data_ptr()) == (model_depth == 2)
        assert np.array_equal(level.numpy(), want)
    ds.close()
    with pytest.raises(RuntimeError):
        ds.level_stack()


def test_level_stack_is_made_in_chunks(monkeypatch):
    stack = make_stack(7, 1, 8, seed=2)
    monkeypatch.setattr(pg.dataset, 'UPLOAD_CHUNK_BYTES', 3 * 64)            # three images at a time: chunks of 3, 3, 1
    ds = pg.DeviceImageDataset(stack, pyramid='direct', device='cpu', model_initial_depth=0)
    assert np.array_equal(ds.level_stack().numpy(), pg.dataset.level_host(stack, 1))


def test_search_follows_the_growth_stage():
    stack = make_stack(9, 3, 16, seed=1)
    ds = pg.DeviceImageDataset(stack, pyramid='chain', device='cpu', model_initial_depth=2)
    nn = pg.metrics.NearestNeighbours(ds, k=2)
    assert nn.device.type == 'cpu'
    for model_depth in (2, 0):
        ds.model_depth = model_depth
        level = ds.level_stack().numpy()
        res = nn.search(_as_samples(level[[7, 3]]))
        assert res['index'][:, 0].tolist() == [7, 3] and res['sqdist'][:, 0].tolist() == [0, 0]
        want = nn_ref.search(level, level[[7, 3]], 2)
        assert np.array_equal(res['sqdist'].numpy(), want[0]) and np.array_equal(res['index'].numpy(), want[1])
    with pytest.raises(ValueError):
        nn.search(torch.zeros(2, 3, 8, 8))                                   # not this stage's resolution


# ------------------------------------------------------------------------------------------------------------- the monitor
class _Z(object):
    """Latents whose ``.cuda()`` stays on the host."""

    def __init__(self, z):
        self.z = z

    def cuda(self):
        return self.z


class _G(object):
    """forward(z) = the samples the test planted, by latent row."""

    def __init__(self, samples, tag):
        self.samples, self.tag, self.calls = samples, tag, 0

    def forward(self, z):
        self.calls += 1
        return self.samples[:z]


class _Ema(object):
    def __init__(self, gs):
        self.gs = gs

    def network(self):
        return self.gs


class _Parallel(object):
    def __init__(self, rank):
        self.rank = rank


class _Trainer(object):
    def __init__(self, G, g_ema=None, parallel=None, cur_nimg=123456):
        self.G, self.g_ema, self.parallel, self.stats, self.cur_nimg = G, g_ema, parallel, {}, cur_nimg


class _Proc(object):
    def __init__(self, device_tensors):
        self.accepts_device_tensors = device_tensors
        self.calls = []

    def __call__(self, batch, description):
        self.calls.append((batch, description))


def _setup(mirror_augment=False, M=12, C=3, r=8, n=6):
    stack = nn_ref.images(M, C, r, seed=5)
    ds = pg.DeviceImageDataset(stack, device='cpu', model_initial_depth=1, mirror_augment=mirror_augment)     # depth 3 = 8x8: the source
    q = nn_ref.images(n, C, r, seed=6)
    q[1] = stack[9]
    q[2] = stack[4][..., ::-1]
    return stack, ds, q, _as_samples(q)


def test_monitor_stats_sheet_and_description():
    stack, ds, q, samples = _setup()
    k = 2
    host_proc, dev_proc = _Proc(False), _Proc(True)
    mon = pg.NNMonitor(ds, lambda n: _Z(n), num_samples=5, k=k, nn_ticks=7, postprocessors=(host_proc, dev_proc))
    assert mon.trigger_interval == [(7, 'epoch'), (1, 'end')] and mon.mirror is False
    tr = _Trainer(_G(samples, 'G'))
    mon.register(tr)
    mon.epoch(1)
    assert tr.G.calls == 1
    sq, ix = nn_ref.search(stack, q[:5], k)
    rms = np.sqrt(sq[:, 0].astype(np.float64) / (3 * 8 * 8))
    assert sorted(tr.stats) == ['nn_rms', 'nn_rms_min']
    assert tr.stats['nn_rms'] == dict(log_name='nn_rms', log_epoch_fields=['{val:.2f}'], val=float(rms.mean()))
    assert tr.stats['nn_rms_min'] == dict(log_name='nn_rms_min', log_epoch_fields=['{val:.2f}'], val=0.0)         # the planted copy
    # one batch of (k + 1)^2 images: sample i, then its k neighbours, row by row of a grid that is k + 1 wide
    (host_batch, host_desc), (dev_batch, dev_desc) = host_proc.calls[0], dev_proc.calls[0]
    assert host_desc == dev_desc == 'nn_000123'
    assert isinstance(host_batch, np.ndarray) and torch.is_tensor(dev_batch) and np.array_equal(host_batch, dev_batch.numpy())
    assert host_batch.shape == ((k + 1) ** 2, 3, 8, 8) and host_batch.dtype == np.float32
    for i in range(k + 1):
        assert np.array_equal(host_batch[(k + 1) * i], samples[i].numpy())
        for j in range(k):
            want = pg.dataset.prepare_host(stack[ix[i, j]], 1.0, (0, 255), (-1, 1))
            assert np.array_equal(host_batch[(k + 1) * i + 1 + j], want)
    assert np.array_equal(host_batch[(k + 1) * 1 + 1], samples[1].numpy())                                        # the copy next to its sample
    mon.end(2)
    assert len(host_proc.calls) == 2 and tr.G.calls == 2
    # no post-processor: statistics only
    quiet = pg.NNMonitor(ds, lambda n: _Z(n), num_samples=6, k=1)
    tr2 = _Trainer(_G(samples, 'G'))
    quiet.register(tr2)
    quiet.epoch(1)
    assert sorted(tr2.stats) == ['nn_rms', 'nn_rms_min']


def test_monitor_mirror_default_comes_from_the_data_set():
    stack, ds, q, samples = _setup(mirror_augment=True)
    mon = pg.NNMonitor(ds, lambda n: _Z(n), num_samples=6, k=2, postprocessors=(_Proc(False),))
    assert mon.mirror is True and pg.NNMonitor(ds, None, mirror=False).mirror is False
    tr = _Trainer(_G(samples, 'G'))
    mon.register(tr)
    mon.epoch(1)
    batch = mon.postprocessors[0].calls[0][0]
    assert np.array_equal(batch[3 * 2 + 1], samples[2].numpy())              # the mirrored training image, shown as it matched
    sq, ix, mr = nn_ref.search_mirror(stack, q, 2)
    assert tr.stats['nn_rms']['val'] == float(np.sqrt(sq[:, 0].astype(np.float64) / 192).mean())


def test_monitor_runs_on_rank_0_only_and_uses_the_smoothed_generator():
    stack, ds, q, samples = _setup()
    for rank in (1, 3):
        tr = _Trainer(_G(samples, 'G'), parallel=_Parallel(rank))
        mon = pg.NNMonitor(ds, lambda n: _Z(n), num_samples=6, k=2, postprocessors=(_Proc(False),))
        mon.register(tr)
        mon.epoch(1)
        mon.end(1)
        assert tr.stats == {} and tr.G.calls == 0 and mon.postprocessors[0].calls == []
    tr = _Trainer(_G(samples, 'G'), parallel=_Parallel(0))
    mon = pg.NNMonitor(ds, lambda n: _Z(n), num_samples=6, k=2)
    mon.register(tr)
    mon.epoch(1)
    assert 'nn_rms' in tr.stats
    other = _as_samples(nn_ref.images(6, 3, 8, seed=77))
    for smoothed, want in ((None, 'Gs'), (True, 'Gs'), (False, 'G')):
        g, gs = _G(samples, 'G'), _G(other, 'Gs')
        tr = _Trainer(g, g_ema=_Ema(gs))
        mon = pg.NNMonitor(ds, lambda n: _Z(n), num_samples=6, k=2, smoothed=smoothed)
        mon.register(tr)
        mon.epoch(1)
        assert (g.calls, gs.calls) == ((0, 1) if want == 'Gs' else (1, 0))
    with pytest.raises(ValueError):
        pg.NNMonitor(ds, None, smoothed=True).register(_Trainer(_G(samples, 'G')))


# -------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_need_no_device():
    u8 = torch.zeros(4, 3, 4, 4, dtype=torch.uint8)
    f32 = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match='device tensor'):
        pg.ops.quantize_u8(f32)
    with pytest.raises(ValueError, match='device tensor'):
        pg.ops.l2dist_u8(u8, u8)
    with pytest.raises(ValueError, match='device tensor'):
        pg.ops.topk_smallest_i64(torch.zeros(2, 4, dtype=torch.int64), 1)
    with pytest.raises(ValueError):
        pg.ops.nn_search_u8(u8, u8, k=1)
    ds = pg.DeviceImageDataset(u8, device='cpu', range_in=(0, 1))
    with pytest.raises(ValueError, match='range_in'):
        pg.metrics.NearestNeighbours(ds)
    for bad in (dict(k=0), dict(k=5), dict(k=17), dict(k=True), dict(drange=(1, 1))):
        with pytest.raises(ValueError):
            pg.metrics.NearestNeighbours(u8, device='cpu', **bad)
    for source in (f32, torch.zeros(4, 4, dtype=torch.uint8), 'stack', None):
        with pytest.raises(ValueError):
            pg.metrics.NearestNeighbours(source, device='cpu')
    nn = pg.metrics.NearestNeighbours(u8, device='cpu')
    for samples in (torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 4, 4), torch.zeros(3, 4, 4), torch.zeros(2, 3, 4, 4, dtype=torch.float64), None):
        with pytest.raises(ValueError):
            nn.search(samples)
    ok = pg.DeviceImageDataset(u8, device='cpu')
    for bad in (dict(k=0), dict(num_samples=3, k=3), dict(num_samples=2.5)):
        with pytest.raises(ValueError):
            pg.NNMonitor(ok, None, **bad)
