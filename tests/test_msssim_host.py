"""Host side of the MS-SSIM metric: the scale table of ``ops.msssim_scales`` and ``plugins.MSSSIMMonitor`` driven by a stub trainer
and a stub metric (no device).  The kernels and ``metrics.MultiScaleSSIM`` are checked on the device (tests/test_msssim_gpu.py)."""
import pytest
import torch

import pggan_amd as pg


def test_scale_table():
    for r, count in ((16, 1), (32, 2), (64, 3), (128, 4), (256, 5), (512, 5), (1024, 5)):
        sides, weights = pg.ops.msssim_scales(r)
        assert sides == [r >> s for s in range(count)] and min(sides) >= 16
        assert len(weights) == count and abs(sum(weights) - 1.0) < 1e-15
    published = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert pg.ops.msssim_scales(64)[1] == [w / sum(published[:3]) for w in published[:3]]
    for bad in (8, 24, 0):
        with pytest.raises(ValueError):
            pg.ops.msssim_scales(bad)


def test_names_and_signatures():
    P, I, L, F = pg._lib.P, pg._lib.I, pg._lib.L, pg._lib.F
    assert pg._lib.SIGNATURES['pg_msssim_scale'] == [P, P, P, P, P, L, I, I, F, F, P]
    assert pg._lib.SIGNATURES['pg_msssim_finish'] == [P, P, P, L, I, I, P]
    assert 'MSSSIMMonitor' in pg.__all__ and pg.plugins.MSSSIMMonitor is pg.MSSSIMMonitor
    assert hasattr(pg.metrics, 'MultiScaleSSIM')
    assert 'the one metric of the paper' not in pg.metrics.__doc__


def test_argument_errors_need_no_device():
    a = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match='device tensor'):
        pg.ops.msssim_pairs(a, a)
    with pytest.raises(ValueError):
        pg.metrics.MultiScaleSSIM(24, 4)
    with pytest.raises(ValueError):
        pg.metrics.MultiScaleSSIM(16, 4, num_channels=2)
    with pytest.raises(ValueError):
        pg.metrics.MultiScaleSSIM(16, 0)
    with pytest.raises(ValueError):
        pg.MSSSIMMonitor(None, num_pairs=0)


class _Z(object):
    """Latents whose ``.cuda()`` stays on the host."""

    def __init__(self, z):
        self.z = z

    def cuda(self):
        return self.z


class _G(object):
    num_channels = 1

    def __init__(self, depth, tag):
        self.depth, self.tag, self.calls = depth, tag, 0

    def forward(self, z):
        self.calls += 1
        return (self.tag, z)


class _Ema(object):
    def __init__(self, gs):
        self.gs = gs

    def network(self):
        return self.gs


class _Parallel(object):
    def __init__(self, rank):
        self.rank = rank


class _Trainer(object):
    def __init__(self, depth=2, g_ema=None, parallel=None):
        self.G = _G(depth, 'G')
        self.g_ema, self.parallel, self.stats = g_ema, parallel, {}


class _Metric(object):
    made = []

    def __init__(self, resolution, num_pairs, num_channels=3, **kw):
        self.resolution, self.num_pairs, self.num_channels, self.kw = resolution, num_pairs, num_channels, kw
        self.fed, self.resets = [], 0
        _Metric.made.append(self)

    def reset(self):
        self.resets += 1
        self.fed = []

    def feed(self, a, b):
        self.fed.append((a, b))

    def result(self):
        return {'msssim': 0.123456, 'std': 0.05, 'scales': [self.resolution], 'terms': [0.2]}


@pytest.fixture()
def stub_metric(monkeypatch):
    _Metric.made = []
    monkeypatch.setattr(pg.metrics, 'MultiScaleSSIM', _Metric)
    return _Metric


def _monitor(**kw):
    drawn = []

    def sample_fn(n):
        drawn.append(n)
        return _Z(('z', len(drawn), n))
    return pg.MSSSIMMonitor(sample_fn, **kw), drawn


def test_monitor_period_stats_and_pairs(stub_metric):
    mon, drawn = _monitor(num_pairs=8, minibatch=3, msssim_ticks=7, quantize=False)
    assert mon.trigger_interval == [(7, 'epoch'), (1, 'end')]
    assert pg.MSSSIMMonitor(None).trigger_interval == [(400, 'epoch'), (1, 'end')] and pg.MSSSIMMonitor(None).num_pairs == 10000
    tr = _Trainer(depth=2)
    mon.register(tr)
    mon.epoch(1)
    (metric,) = stub_metric.made
    assert (metric.resolution, metric.num_pairs, metric.num_channels, metric.kw) == (16, 8, 1, {'quantize': False})
    assert drawn == [3, 3, 3, 3, 2, 2] and tr.G.calls == 6                      # two passes per round, on independent latents
    assert [(a[1][1], b[1][1]) for a, b in metric.fed] == [(1, 2), (3, 4), (5, 6)]
    assert all(a[0] == 'G' and b[0] == 'G' for a, b in metric.fed)
    assert sorted(tr.stats) == ['msssim', 'msssim_std']
    st = tr.stats['msssim']
    assert st['log_name'] == 'msssim' and st['log_epoch_fields'] == ['{val:.4f}'] and st['val'] == 0.123456
    assert st['log_epoch_fields'][0].format(**st) == '0.1235'
    assert tr.stats['msssim_std'] == dict(log_name='msssim_std', log_epoch_fields=['{val:.4f}'], val=0.05)
    mon.end(2)                                                                 # the same metric object, reset, at the same stage
    assert len(stub_metric.made) == 1 and metric.resets == 2 and len(metric.fed) == 3
    tr.G.depth = 3                                                             # a new stage: a new metric
    mon.epoch(3)
    assert [m.resolution for m in stub_metric.made] == [16, 32]


def test_monitor_writes_nothing_below_16_and_off_rank_0(stub_metric):
    for tr in (_Trainer(depth=1), _Trainer(depth=0), _Trainer(depth=2, parallel=_Parallel(1))):
        mon, drawn = _monitor(num_pairs=4, minibatch=2)
        mon.register(tr)
        mon.epoch(1)
        mon.end(1)
        assert tr.stats == {} and drawn == [] and tr.G.calls == 0
    assert stub_metric.made == []
    tr = _Trainer(depth=2, parallel=_Parallel(0))
    mon, _ = _monitor(num_pairs=4, minibatch=2)
    mon.register(tr)
    mon.epoch(1)
    assert 'msssim' in tr.stats


def test_monitor_measures_the_smoothed_generator(stub_metric):
    gs = _G(2, 'Gs')
    for smoothed, want in ((None, 'Gs'), (True, 'Gs'), (False, 'G')):
        tr = _Trainer(depth=2, g_ema=_Ema(gs))
        mon, _ = _monitor(num_pairs=2, minibatch=2, smoothed=smoothed)
        mon.register(tr)
        mon.epoch(1)
        assert stub_metric.made[-1].fed[0][0][0] == want
    plain = _Trainer(depth=2)
    with pytest.raises(ValueError):
        pg.MSSSIMMonitor(None, smoothed=True).register(plain)
    pg.MSSSIMMonitor(None, smoothed=None).register(plain)
    pg.MSSSIMMonitor(None, smoothed=False).register(plain)
