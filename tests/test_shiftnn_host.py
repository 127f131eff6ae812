"""Host side of the shift-invariant window search: ``metrics.ShiftNearestNeighbours(device='cpu')`` (the numpy twin of the device path)
against the brute force of tests/shiftnn_ref.py, ``ops.shift_segments``, the mirror merge, ``plugins.ShiftNNMonitor`` over a host-mode
strip data set with a stub trainer, and the argument errors that need no device.  The kernels are checked on the device
(tests/test_shiftnn_gpu.py).  Every comparison is exact."""
import numpy as np
import pytest
import torch

import shiftnn_ref

import pggan_amd as pg


def _as_samples(images_u8, drange=(-1, 1)):
    """fp32 images in ``drange`` whose 0..255 levels are exactly ``images_u8`` (the data set's own range change)."""
    return torch.from_numpy(pg.dataset.prepare_host(images_u8, 1.0, (0, 255), drange))


def _host_level(strips):
    return pg.dataset.StripLevel.pack(strips, 'cpu')


def test_names_signatures_and_constants():
    P, I, L = pg._lib.P, pg._lib.I, pg._lib.L
    assert pg._lib.SHIFT_SIGNATURES == {'pg_shift_l2min_u8': [P, P, L, I, I, P, I, I, P, L, L, P, P]}
    assert pg._lib.SHIFT_CONSTANTS == {'PG_SHIFT_POS_BITS': 16, 'PG_SHIFT_MAX_QUERIES': 64, 'PG_SHIFT_TILE': 128, 'PG_SHIFT_SEGTAB_WORDS': 2}
    assert 'pg_shift_l2min_u8' not in pg._lib.SIGNATURES and not any(n.startswith('PG_SHIFT') for n in pg._lib.CONSTANTS)
    assert pg._lib.ABI_VERSION == 27                                         # additive: the version stays
    assert pg.ops.SHIFT_POS_BITS == shiftnn_ref.POS_BITS and pg.ops.SHIFT_MAX_QUERIES == pg.ops.NN_MAX_QUERIES
    assert pg.ShiftNNMonitor is pg.plugins.ShiftNNMonitor and pg.ShiftNearestNeighbours is pg.metrics.ShiftNearestNeighbours
    assert 'ShiftNNMonitor' in pg.__all__ and 'ShiftNearestNeighbours' in pg.__all__


@pytest.mark.parametrize('S,seg', [(4, 1), (4, 3), (4, None), (8, 5), (16, 2 * 53), (16, None)])
def test_segment_table(S, seg):
    cols = [S, S + 1, S + 37]
    strip, start, first = pg.ops.shift_segments(cols, S, seg)
    want = shiftnn_ref.segments(cols, S, S if seg is None else seg)
    assert strip.dtype == start.dtype == first.dtype == np.int64
    assert strip.tolist() == [m for m, _, _ in want] and start.tolist() == [g0 for _, g0, _ in want]
    assert first.tolist() == [sum(1 for m, _, _ in want if m < i) for i in range(len(cols) + 1)]
    # the segments of a strip cover its starts exactly once
    for m, T in enumerate(cols):
        covered = []
        for mm, g0, n in want:
            if mm == m:
                covered += list(range(g0, g0 + n))
        assert covered == list(range(T - S + 1))


@pytest.mark.parametrize('C,S', [(1, 4), (2, 4), (3, 8), (2, 16)])
@pytest.mark.parametrize('seg', [1, 3, None, 1000])
def test_twin_keys_equal_the_reference(C, S, seg):
    cols = [S, S + 1, S + 37]
    strips = shiftnn_ref.strips(cols, C, S, seed=11)
    q = shiftnn_ref.queries(5, C, S, seed=12)
    q[1] = strips[2][:, :, 7:7 + S]                                          # a copy at an odd start
    got = pg.metrics._shift_keys_host(strips, q, S if seg is None else seg)
    want = shiftnn_ref.keys(strips, q, S if seg is None else seg)
    assert got.dtype == np.int64 and np.array_equal(got, want)


@pytest.mark.parametrize('mirror', [False, True])
def test_host_search_equals_the_reference(mirror):
    C, S, k, seg = 2, 8, 4, 5
    strips = shiftnn_ref.strips([S + 30, S, S + 13], C, S, seed=21)
    strips[2][:, :, 3:3 + S] = strips[0][:, :, 17:17 + S]                     # the same window in two strips: the lower segment first
    q = shiftnn_ref.queries(6, C, S, seed=22)
    q[2] = strips[0][:, :, 17:17 + S]
    q[3] = strips[0][:, :, 9:9 + S][..., ::-1]                               # a time-reversed copy
    nn = pg.metrics.ShiftNearestNeighbours(_host_level(strips), k=k, mirror=mirror, seg=seg)
    assert nn.device.type == 'cpu'
    res = nn.search(_as_samples(q))
    for name, dtype in (('strip', torch.int64), ('start', torch.int64), ('sqdist', torch.int64), ('rms', torch.float64), ('mirrored', torch.bool)):
        assert res[name].dtype == dtype and tuple(res[name].shape) == (6, k)
    strip, start, sq = shiftnn_ref.search(strips, q, seg, k)
    if not mirror:
        assert np.array_equal(res['strip'].numpy(), strip) and np.array_equal(res['start'].numpy(), start)
        assert np.array_equal(res['sqdist'].numpy(), sq) and not res['mirrored'].any()
        assert res['sqdist'][2, :2].tolist() == [0, 0] and res['strip'][2, :2].tolist() == [0, 2] and res['start'][2, :2].tolist() == [17, 3]
    else:
        # the merge, stated independently: all 2k candidates of a sample sorted by (sqdist, segment, start, mirrored)
        strip_m, start_m, sq_m = shiftnn_ref.search(strips, q[..., ::-1], seg, k)
        segs = shiftnn_ref.segments([s.shape[2] for s in strips], S, seg)
        seg_of = lambda m, u: [i for i, (mm, g0, n) in enumerate(segs) if mm == m and g0 <= u < g0 + n][0]
        for i in range(6):
            cand = [(int(sq[i, j]), seg_of(strip[i, j], start[i, j]), int(start[i, j]), False, int(strip[i, j])) for j in range(k)]
            cand += [(int(sq_m[i, j]), seg_of(strip_m[i, j], start_m[i, j]), int(start_m[i, j]), True, int(strip_m[i, j])) for j in range(k)]
            cand.sort()
            assert res['sqdist'][i].tolist() == [c[0] for c in cand[:k]] and res['start'][i].tolist() == [c[2] for c in cand[:k]]
            assert res['mirrored'][i].tolist() == [c[3] for c in cand[:k]] and res['strip'][i].tolist() == [c[4] for c in cand[:k]]
        assert res['sqdist'][3, 0] == 0 and bool(res['mirrored'][3, 0]) and (res['strip'][3, 0], res['start'][3, 0]) == (0, 9)
    assert np.array_equal(res['rms'].numpy(), np.sqrt(res['sqdist'].numpy().astype(np.float64) / (C * S * S)))
    # the windows the result names
    near = nn.neighbours(res)
    assert tuple(near.shape) == (6, k, C, S, S) and near.dtype == torch.float32
    for i in range(6):
        for j in range(k):
            w = strips[int(res['strip'][i, j])][:, :, int(res['start'][i, j]):int(res['start'][i, j]) + S]
            w = w[..., ::-1] if bool(res['mirrored'][i, j]) else w
            assert np.array_equal(near[i, j].numpy(), pg.dataset.prepare_host(np.ascontiguousarray(w), 1.0, (0, 255), (-1, 1)))


def _strip_dataset(pyramid='chain', depth=2, R=16, cols=(16 * 5, 16 * 3 + 7), C=2, seed=31, **kw):
    strips = shiftnn_ref.strips(list(cols), C, R, seed=seed)
    return strips, pg.DeviceStripDataset(strips, device='cpu', model_initial_depth=depth, pyramid=pyramid, **kw)   # depth + 2 = log2(side)


@pytest.mark.parametrize('pyramid', ['chain', 'direct'])
@pytest.mark.parametrize('depth', [1, 2])
def test_data_set_stage_and_bound_by_the_non_overlapping_search(pyramid, depth):
    """The search follows the stage; whenever the segments cover all starts, the best shift distance of a sample is at most the best
    distance over the non-overlapping windows of ``level_stack()`` (those windows are among the searched ones)."""
    R = 16
    strips, ds = _strip_dataset(pyramid, depth, R)
    S = 4 << depth
    scale = 4 - (depth + 2)
    nn = pg.metrics.ShiftNearestNeighbours(ds, k=2)
    level, got_scale = nn.level()
    assert got_scale == scale and [s.shape for s in level] == [(2, S, t >> scale) for t in ds.lengths]
    if scale:
        want = [pg.dataset.level_host(s[:, :, :t], scale, (0, 255)) for s, t in zip(strips, ds.lengths)]    # one level down: both pyramids agree
        assert all(np.array_equal(a, b) for a, b in zip(level, want))
        assert nn.level()[0] is level                                        # made once per stage and kept
    u = 5                                                                    # a stored column that is no multiple of S
    window = level[1][:, :, u:u + S]
    other = shiftnn_ref.queries(3, 2, S, seed=32)
    q = np.concatenate([window[None], other])
    res = nn.search(_as_samples(q))
    assert res['sqdist'][0, 0] == 0 and res['strip'][0, 0] == 1 and res['start'][0, 0] == u << scale
    assert all(int(s) % (1 << scale) == 0 for s in res['start'].reshape(-1))
    plain = pg.metrics.NearestNeighbours(ds, k=1).search(_as_samples(q))
    assert plain['sqdist'][0, 0] > 0                                         # the non-overlapping search does not see the copy
    assert bool((res['sqdist'][:, 0] <= plain['sqdist'][:, 0]).all())
    strip, start, sq = shiftnn_ref.search(level, q, S, 2)
    assert np.array_equal(res['sqdist'].numpy(), sq) and np.array_equal(res['start'].numpy(), start << scale)
    ds.model_depth = 2 if depth == 1 else 1                                  # the stage moves: the next search reads the new level
    assert nn.level()[0][0].shape[1] == 4 << ds.model_depth


# ------------------------------------------------------------------------------------------------------------- the monitor
class _Z(object):
    """Latents whose ``.cuda()`` stays on the host."""

    def __init__(self, z):
        self.z = z

    def cuda(self):
        return self.z


class _G(object):
    """forward(z) = the samples the test planted, by latent row."""

    def __init__(self, samples):
        self.samples, self.calls = samples, 0

    def forward(self, z):
        self.calls += 1
        return self.samples[:z]


class _Parallel(object):
    def __init__(self, rank):
        self.rank = rank


class _Trainer(object):
    def __init__(self, G, parallel=None, cur_nimg=123456):
        self.G, self.g_ema, self.parallel, self.stats, self.cur_nimg = G, None, parallel, {}, cur_nimg


class _Proc(object):
    def __init__(self, device_tensors):
        self.accepts_device_tensors = device_tensors
        self.calls = []

    def __call__(self, batch, description):
        self.calls.append((batch, description))


def test_monitor_stats_sheet_and_description():
    R, k = 16, 2
    strips, ds = _strip_dataset('chain', 2, R)
    kept = [s[:, :, :t] for s, t in zip(strips, ds.lengths)]
    q = shiftnn_ref.queries(5, 2, R, seed=41)
    q[1] = kept[0][:, :, 21:21 + R]                                          # a copy at a start NNMonitor cannot see
    samples = _as_samples(q)
    host_proc, dev_proc = _Proc(False), _Proc(True)
    mon = pg.ShiftNNMonitor(ds, lambda n: _Z(n), num_samples=5, k=k, nn_ticks=7, postprocessors=(host_proc, dev_proc))
    assert mon.trigger_interval == [(7, 'epoch'), (1, 'end')] and mon.mirror is False
    tr = _Trainer(_G(samples))
    mon.register(tr)
    mon.epoch(1)
    assert tr.G.calls == 1
    strip, start, sq = shiftnn_ref.search(kept, q, R, k)
    rms = np.sqrt(sq[:, 0].astype(np.float64) / (2 * R * R))
    assert sorted(tr.stats) == ['nn_shift_rms', 'nn_shift_rms_min']
    assert tr.stats['nn_shift_rms'] == dict(log_name='nn_shift_rms', log_epoch_fields=['{val:.2f}'], val=float(rms.mean()))
    assert tr.stats['nn_shift_rms_min'] == dict(log_name='nn_shift_rms_min', log_epoch_fields=['{val:.2f}'], val=0.0)
    (host_batch, host_desc), (dev_batch, dev_desc) = host_proc.calls[0], dev_proc.calls[0]
    assert host_desc == dev_desc == 'nnshift_000123'
    assert isinstance(host_batch, np.ndarray) and torch.is_tensor(dev_batch) and np.array_equal(host_batch, dev_batch.numpy())
    assert host_batch.shape == ((k + 1) ** 2, 2, R, R) and host_batch.dtype == np.float32
    for i in range(k + 1):
        assert np.array_equal(host_batch[(k + 1) * i], samples[i].numpy())
        for j in range(k):
            w = np.ascontiguousarray(kept[strip[i, j]][:, :, start[i, j]:start[i, j] + R])
            assert np.array_equal(host_batch[(k + 1) * i + 1 + j], pg.dataset.prepare_host(w, 1.0, (0, 255), (-1, 1)))
    assert np.array_equal(host_batch[(k + 1) * 1 + 1], samples[1].numpy())   # the copy next to its sample
    # rank 0 evaluates
    tr1 = _Trainer(_G(samples), parallel=_Parallel(1))
    other = pg.ShiftNNMonitor(ds, lambda n: _Z(n), num_samples=5, k=k)
    other.register(tr1)
    other.epoch(1)
    other.end(1)
    assert tr1.stats == {} and tr1.G.calls == 0
    # the mirror default comes from the data set
    _, dsm = _strip_dataset('chain', 2, R, mirror_augment=True)
    assert pg.ShiftNNMonitor(dsm, None).mirror is True and pg.ShiftNNMonitor(dsm, None, mirror=False).mirror is False


# -------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_need_no_device():
    S = 4
    strips = shiftnn_ref.strips([S + 3, S], 1, S, seed=51)
    level = _host_level(strips)
    q = torch.zeros(2, 1, S, S, dtype=torch.uint8)
    with pytest.raises(ValueError, match='device tensor'):
        pg.ops.shift_l2min_u8(level, q)
    with pytest.raises(ValueError, match='device tensor'):
        pg.ops.shift_table(level)
    for bad in (dict(cols=[S, S - 1], S=S), dict(cols=[], S=S), dict(cols=[8], S=3), dict(cols=[8], S=2), dict(cols=[4096], S=2048),
                dict(cols=[8], S=S, seg=0), dict(cols=[8], S=S, seg=(1 << 16) + 1), dict(cols=[8], S=S, seg=1.5), dict(cols=[8], S=S, seg=True)):
        with pytest.raises(ValueError):
            pg.ops.shift_segments(**bad)
    assert len(pg.ops.shift_segments([1 << 17], S, 1 << 16)[0]) == 2         # the largest segment is allowed
    _, ds = _strip_dataset(range_in=(0, 1))
    with pytest.raises(ValueError, match='range_in'):
        pg.metrics.ShiftNearestNeighbours(ds)
    for bad in (dict(k=0), dict(k=6), dict(k=17), dict(k=True), dict(drange=(1, 1)), dict(seg=0), dict(seg=1 << 17)):   # G = 2 segments
        with pytest.raises(ValueError):
            pg.metrics.ShiftNearestNeighbours(level, **bad)
    for source in (torch.zeros(4, 1, 4, 4, dtype=torch.uint8), strips, 'level', None):
        with pytest.raises(ValueError):
            pg.metrics.ShiftNearestNeighbours(source)
    nn = pg.metrics.ShiftNearestNeighbours(level)
    for samples in (torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 4, 4), torch.zeros(1, 4, 4), torch.zeros(2, 1, 4, 4, dtype=torch.float64), None):
        with pytest.raises(ValueError):
            nn.search(samples)
    _, ok = _strip_dataset()
    for bad in (dict(k=0), dict(num_samples=3, k=3), dict(num_samples=2.5)):
        with pytest.raises(ValueError):
            pg.ShiftNNMonitor(ok, None, **bad)
