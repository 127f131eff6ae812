"""Pins the CPU statement of the sliced Wasserstein metric (tests/swd_ref.py) that the device path is held against, and the host side of
metrics.SlicedWasserstein / plugins.SWDMonitor (argument checks, the stages without a pyramid level).  No GPU."""
import types

import numpy as np
import pytest
import torch

import swd_ref


def _images(seed, n=4, res=32, dtype=torch.float64):
    """smooth-ish images: 8x8 Gaussian noise repeated x4 in both directions plus 0.3 * noise (res = 32)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(n, 3, res // 4, res // 4, generator=g, dtype=torch.float64)
    x = low.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3) + 0.3 * torch.randn(n, 3, res, res, generator=g, dtype=torch.float64)
    return x.to(dtype)


def _centres(seed, n, P, sizes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, s - 3, (n * P, 2), generator=g, dtype=torch.int32) for s in sizes]


def _directions(seed, R=2, K=16):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(R, 147, K, generator=g, dtype=torch.float64)
    return d / d.pow(2).sum(dim=1, keepdim=True).sqrt()


@pytest.mark.parametrize('dtype,tol', [(torch.float64, 1e-6), (torch.float32, 1e-6)])
def test_pyramid_of_a_constant_image(dtype, tol):
    x = torch.full((2, 3, 64, 64), 0.625, dtype=dtype)
    assert float((swd_ref.down(x) - 0.625).abs().max()) <= tol
    assert float((swd_ref.up(x) - 0.625).abs().max()) <= tol
    levels = swd_ref.lap_pyramid(x)
    assert [l.shape[-1] for l in levels] == [64, 32, 16]
    for l in levels[:-1]:
        assert float(l.abs().max()) <= tol
    assert float((levels[-1] - 0.625).abs().max()) <= tol


def test_down_and_up_equal_scipy_mirror_convolution():
    ndimage = pytest.importorskip('scipy.ndimage')
    rs = np.random.RandomState(3)
    img = rs.randn(16, 16)
    f = np.array([1, 4, 6, 4, 1], np.float64) / 16
    k = np.outer(f, f)
    x = torch.tensor(img)[None, None].repeat(1, 3, 1, 1)
    ref_down = ndimage.convolve(img, k, mode='mirror')[::2, ::2]
    assert np.abs(swd_ref.down(x)[0, 1].numpy() - ref_down).max() <= 1e-12
    z = np.zeros((32, 32))
    z[::2, ::2] = img
    ref_up = ndimage.convolve(z, 4 * k, mode='mirror')
    assert np.abs(swd_ref.up(x)[0, 2].numpy() - ref_up).max() <= 1e-12


def test_descriptors_are_the_slices_in_channel_dy_dx_order():
    lv = torch.arange(2 * 3 * 16 * 16, dtype=torch.float64).view(2, 3, 16, 16)
    c = torch.tensor([[3, 3], [12, 3], [3, 12], [12, 12], [5, 9], [7, 4]], dtype=torch.int32)
    d = swd_ref.descriptors(lv, c, 3)
    assert d.shape == (6, 3, 7, 7)
    assert float(d[4, 2, 0, 6]) == float(lv[1, 2, 9 - 3, 5 + 3])           # descriptor 4 belongs to image 4 // 3, (x, y) = (5, 9)
    assert float(d[1, 0, 3, 3]) == float(lv[0, 0, 3, 12])


def test_identical_sets_give_exactly_zero():
    a = _images(1)
    cs = _centres(2, 4, 8, [32, 16])
    r = swd_ref.swd(a, a.clone(), cs, _directions(3), 8)
    assert r['swd'] == [0.0, 0.0] and r['mean'] == 0.0


def test_a_constant_shift_of_one_set_is_normalised_away():
    a, b = _images(1), _images(5)
    cs = _centres(2, 4, 8, [32, 16])
    dirs = _directions(3)
    r0 = swd_ref.swd(a, b, cs, dirs, 8)
    r1 = swd_ref.swd(a, b + 0.75, cs, dirs, 8)
    assert min(r0['swd']) > 1.0                                            # (two different sets are apart)
    for v0, v1 in zip(r0['swd'], r1['swd']):
        assert abs(v0 - v1) <= 1e-9


def test_sliced_wasserstein_argument_errors():
    import pggan_amd as pg
    SW = pg.metrics.SlicedWasserstein
    for bad in (8, 24, 0):
        with pytest.raises(ValueError):
            SW(bad, 4)
    with pytest.raises(ValueError):
        SW(32, 0)
    with pytest.raises(ValueError):
        SW(32, 4, patches_per_image=0)
    with pytest.raises(ValueError):
        SW(32, 4, dir_repeats=0)
    with pytest.raises(ValueError):
        SW(32, 4, dirs_per_repeat=-1)
    with pytest.raises(ValueError):
        SW(32, 4, num_channels=1)                                          # single-channel networks are out of contract
    with pytest.raises(ValueError):
        SW(128, 1 << 16, patches_per_image=128)                            # 2^23 descriptors: above the sort's limit
    assert pg.metrics.swd_levels(128) == [128, 64, 32, 16]


def test_swd_monitor_skips_stages_below_16():
    import pggan_amd as pg

    def never(n):
        raise AssertionError('an 8x8 stage has no pyramid level: nothing may be drawn or generated')

    mon = pg.SWDMonitor(never, never, num_images=8, minibatch=4, swd_ticks=3, patches_per_image=8)
    assert isinstance(mon, pg.Plugin) and mon.trigger_interval == [(3, 'epoch'), (1, 'end')]
    trainer = types.SimpleNamespace(stats={'kimg_stat': 1}, parallel=None, G=types.SimpleNamespace(depth=1, forward=never), cur_nimg=0)
    mon.register(trainer)
    mon.epoch(1)
    mon.end(1)
    assert trainer.stats == {'kimg_stat': 1}
    # a replica of a data-parallel run never evaluates, whatever the stage
    trainer.parallel, trainer.G.depth = types.SimpleNamespace(rank=1), 3
    mon.epoch(2)
    assert trainer.stats == {'kimg_stat': 1}


def test_swd_monitor_keeps_one_metric_object_at_a_time(monkeypatch):
    """The descriptor buffers of a stage are gigabytes at the default size: when the stage changes, the last stage's object goes."""
    import gc
    import weakref
    import pggan_amd as pg

    class FakeMetric(object):
        made = []

        def __init__(self, resolution, num_images, **kw):
            self.resolution, self.num_images, self.kw = resolution, num_images, kw
            self.fed = {'real': 0, 'fake': 0}
            FakeMetric.made.append(weakref.ref(self))

        def reset(self):
            self.fed = {'real': 0, 'fake': 0}

        def feed_real(self, batch):
            self.fed['real'] += batch.shape[0]

        def feed_fake(self, batch):
            self.fed['fake'] += batch.shape[0]

        def result(self):
            assert self.fed == {'real': self.num_images, 'fake': self.num_images}
            levels = pg.metrics.swd_levels(self.resolution)
            return {'levels': levels, 'swd': [float(s) for s in levels], 'mean': 1.5}

    monkeypatch.setattr(pg.metrics, 'SlicedWasserstein', FakeMetric)
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)
    G = types.SimpleNamespace(depth=2, forward=lambda z: torch.zeros(z.shape[0], 3, 4 * 2 ** G.depth, 4 * 2 ** G.depth))
    trainer = types.SimpleNamespace(stats={}, parallel=None, G=G, cur_nimg=0)
    mon = pg.SWDMonitor(lambda n: torch.zeros(n, 3, 4 * 2 ** G.depth, 4 * 2 ** G.depth), lambda n: torch.zeros(n, 8), num_images=7,
                        minibatch=3, swd_ticks=1, patches_per_image=8)
    mon.register(trainer)
    mon.epoch(1)
    mon.epoch(2)
    assert len(FakeMetric.made) == 1 and FakeMetric.made[0]().kw == {'patches_per_image': 8}    # same stage: the same object, reset
    assert set(trainer.stats) == {'swd', 'swd_16'} and trainer.stats['swd']['val'] == 1.5 and trainer.stats['swd_16']['val'] == 16.0
    G.depth = 3
    mon.epoch(3)
    gc.collect()
    assert len(FakeMetric.made) == 2 and FakeMetric.made[0]() is None and FakeMetric.made[1]().resolution == 32
    assert set(trainer.stats) == {'swd', 'swd_16', 'swd_32'}
