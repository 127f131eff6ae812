"""The MS-SSIM metric on the MI355X (csrc/msssim.hip through ops.msssim_pairs, metrics.MultiScaleSSIM, plugins.MSSSIMMonitor) against
its torch-CPU statement tests/msssim_ref.py: fp64 for the values, fp32 operation for operation for the quantisation step.  Shapes are
the smallest at which each part can go wrong: less than a tile (16), a pooled side of 16 with an odd batch (32), three scales (64)
and the published five (256), where every valid side 246, 118, 54, 22, 6 is off the 32-wide tile grid.

BOUND: the largest absolute error of the device against the fp64 reference over exactly these inputs (both kinds of image, every
shape, values and every per-scale term, with and without quantisation) was measured on an MI355X as 8.835e-7 (the cs term of the 64x64
scale of the smooth (2, 3, 256) case; docs/experiments_msssim.md).  The asserted bound is 4 x that, rounded up to one digit: 4e-6 -- the
margin is for summation-order differences between machines of the same definition -- under the cap of 1e-4, the resolution the metric is
read at.  Every case prints its error before it asserts."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msssim_ref as ref

pytestmark = pytest.mark.gpu

MEASURED = 8.835e-7      # largest device error on these inputs (docs/experiments_msssim.md)
BOUND = 4e-6             # 4 x MEASURED, rounded up to one digit; may never exceed 1e-4
SHAPES = [(1, 1, 16), (3, 3, 32), (2, 1, 64), (2, 3, 256)]
KINDS = ['smooth', 'flat']


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _smooth(n, C, R, g):
    """Bilinear-upsampled low-resolution noise blended with pixel noise, values in 0.3 .. 0.6."""
    low = torch.rand(n, C, max(R // 8, 2), max(R // 8, 2), generator=g, dtype=torch.float32)
    up = F.interpolate(low, size=(R, R), mode='bilinear', align_corners=False)
    return 0.3 + 0.3 * (0.75 * up + 0.25 * torch.rand(n, C, R, R, generator=g, dtype=torch.float32))


_inputs, _refs = {}, {}


def inputs(shape, kind):
    """The pair of fp32 batches of a case, made once.  'smooth': b shares half of a's structure, so that the values lie well inside
    (0, 1); 'flat': two independent near-flat images, the worst case for the cancellation in the variances."""
    key = (shape, kind)
    if key not in _inputs:
        n, C, R = shape
        g = _gen(1000 * R + 10 * n + C + (0 if kind == 'smooth' else 5))
        if kind == 'smooth':
            a = _smooth(n, C, R, g)
            b = (0.5 * a + 0.5 * _smooth(n, C, R, g)).contiguous()
        else:
            a = 0.9 + 0.004 * torch.randn(n, C, R, R, generator=g, dtype=torch.float32)
            b = 0.9 + 0.004 * torch.randn(n, C, R, R, generator=g, dtype=torch.float32)
        _inputs[key] = (a, b)
    return _inputs[key]


def reference(shape, kind, quantize=True):
    key = (shape, kind, quantize)
    if key not in _refs:
        a, b = inputs(shape, kind)
        _refs[key] = ref.msssim_pairs(a.double(), b.double(), quantize=quantize)
    return _refs[key]


def _err(got, want):
    return float((got.cpu().double() - want).abs().max())


# ------------------------------------------------------------------------------------------------- against the fp64 reference
@pytest.mark.parametrize('quantize', [True, False])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_against_reference(pg, shape, kind, quantize):
    a, b = inputs(shape, kind)
    want_v, want_t = reference(shape, kind, quantize)
    values, terms = pg.ops.msssim_pairs(a.cuda(), b.cuda(), quantize=quantize)
    assert values.dtype == torch.float64 and tuple(values.shape) == (shape[0],)
    assert tuple(terms.shape) == (shape[0], len(ref.scales(shape[2])[0]))
    ev, et = _err(values, want_v), _err(terms, want_t)
    print('msssim %s %s quantize=%s: values %s  max abs err values %.3e terms %.3e'
          % (shape, kind, quantize, [round(float(v), 4) for v in want_v], ev, et))
    assert max(ev, et) <= BOUND
    if kind == 'smooth':
        assert 0.02 < float(want_v.min()) and float(want_v.max()) < 0.98       # the case is not degenerate


# ------------------------------------------------------------------------------------------------- quantisation
@pytest.mark.parametrize('shape', [(3, 3, 32), (2, 3, 256)])
def test_pooled_quantised_image_matches_the_fp32_reference(pg, shape):
    a, b = inputs(shape, 'smooth')
    scratch = pg.ops.MSSSIMScratch(shape[0], shape[1], shape[2], 'cuda')
    pg.ops.msssim_pairs(a.cuda(), b.cuda(), scratch=scratch)
    _, _, pooled = ref.msssim_pairs(a, b, return_pooled=True)                # fp32: the mirror
    for got, want in zip(scratch.pooled[0], pooled[0]):
        got = got.cpu()
        assert got.shape == want.shape and len(torch.unique(want)) > 50
        ulp = torch.from_numpy(np.spacing(want.abs().numpy()))
        assert bool(((got - want).abs() <= ulp).all()), float((got - want).abs().max())
    # the coarser scales are means of means of the same values: exact too, up to the summation order both sides share
    for lvl in range(1, len(pooled)):
        for got, want in zip(scratch.pooled[lvl], pooled[lvl]):
            assert float((got.cpu() - want).abs().max()) <= 255 * 2.0 ** -22


@pytest.mark.parametrize('C', [1, 3])
def test_quantisation_is_the_image_grid_path(pg, C):
    """Values exactly on .5 boundaries and outside ``drange`` reach the same uint8 levels as the sample-grid path.  Every pixel of the
    16x16 image is repeated 2x2, so the pooled image of the first scale IS the quantised image."""
    # drange (-255, 255): the scale is 0.5 and x = 2 m + 1 - 255 lands exactly on m + 0.5
    m = torch.arange(256, dtype=torch.float32)
    on_boundary = (2 * m + 1 - 255).view(1, 1, 16, 16).repeat(1, C, 1, 1)
    on_boundary[0, 0, 0, :4] = torch.tensor([-300.0, -255.5, 255.5, 1e6])
    # the default drange: the fp32 neighbours of every boundary, whichever side the two roundings put them on
    near = ((2 * m + 1) / 255 - 1).view(1, 1, 16, 16).repeat(1, C, 1, 1)
    if C == 3:
        near[0, 1] = torch.nextafter(near[0, 1], torch.tensor(2.0))
        near[0, 2] = torch.nextafter(near[0, 2], torch.tensor(-2.0))
    near[0, 0, 0, :3] = torch.tensor([-1.2, 1.0001, 7.0])
    for low, drange in ((on_boundary, (-255, 255)), (near, (-1, 1))):
        x = low.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).contiguous().cuda()
        scratch = pg.ops.MSSSIMScratch(1, C, 32, 'cuda')
        values, _ = pg.ops.msssim_pairs(x, x.clone(), drange=drange, scratch=scratch)
        grid = pg.ops.image_grid_u8(low.cuda(), drange=drange)              # [16,16,C] uint8
        want = grid.permute(2, 0, 1).float().cpu()
        for got in scratch.pooled[0]:
            assert torch.equal(got[0].cpu(), want)
        assert torch.equal(want, ref.quantise(low, drange)[0])               # and the fp32 mirror agrees with both
        assert float(values[0]) == 1.0
    assert want.min() == 0 and want.max() == 255


# ------------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_identical_images_give_exactly_one_and_runs_are_bit_equal(pg, shape, kind):
    a, b = (t.cuda() for t in inputs(shape, kind))
    for quantize in (True, False):
        values, terms = pg.ops.msssim_pairs(a, a.clone(), quantize=quantize)
        assert bool((values == 1.0).all()) and bool((terms == 1.0).all())
    v1, t1 = pg.ops.msssim_pairs(a, b)
    v2, t2 = pg.ops.msssim_pairs(a, b)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)
    # a <-> b: the same value up to rounding
    v3, t3 = pg.ops.msssim_pairs(b, a)
    assert _err(v3, v1.cpu()) <= BOUND and _err(t3, t1.cpu()) <= BOUND
    # a pair's value does not depend on what else is in the batch
    for i in range(shape[0]):
        vi, ti = pg.ops.msssim_pairs(a[i:i + 1].contiguous(), b[i:i + 1].contiguous())
        assert torch.equal(vi[0], v1[i]) and torch.equal(ti[0], t1[i])


def test_unrelated_noise_gives_exactly_zero(pg):
    g = _gen(0)
    a = torch.rand(8, 1, 16, 16, generator=g, dtype=torch.float32) * 2 - 1
    b = torch.rand(8, 1, 16, 16, generator=g, dtype=torch.float32) * 2 - 1
    want_v, want_t = ref.msssim_pairs(a.double(), b.double())
    negative = want_t[:, 0] < 0
    assert int(negative.sum()) >= 1 and float(want_t[:, 0].abs().min()) > 100 * BOUND      # no sign hangs on rounding
    values, terms = pg.ops.msssim_pairs(a.cuda(), b.cuda())
    values, terms = values.cpu(), terms.cpu()
    assert bool(torch.isfinite(values).all()) and bool((values[negative] == 0.0).all()) and bool((values[~negative] > 0.0).all())
    assert bool((terms[negative, 0] < 0).all())
    assert _err(values, want_v) <= BOUND and _err(terms, want_t) <= BOUND


# ------------------------------------------------------------------------------------------------- the metric object
def test_metric_object_takes_any_split(pg):
    g = _gen(21)
    a = _smooth(4, 3, 32, g)
    b = (0.5 * a + 0.5 * _smooth(4, 3, 32, g)).contiguous()
    a, b = a.cuda(), b.cuda()
    whole = pg.metrics.MultiScaleSSIM(32, 4)
    assert not whole.complete
    whole.feed(a, b)
    assert whole.complete
    res = whole.result()
    split = pg.metrics.MultiScaleSSIM(32, 4)
    for lo, hi in ((0, 1), (1, 3), (3, 4)):
        split.feed(a[lo:hi].contiguous(), b[lo:hi].contiguous())
    assert split.result() == res
    want_v, want_t = ref.msssim_pairs(a.cpu().double(), b.cpu().double())
    mean, std = ref.summary(want_v)
    assert res['scales'] == [32, 16] and len(res['terms']) == 2
    assert abs(res['msssim'] - mean) <= BOUND and abs(res['std'] - std) <= BOUND and std > 0
    assert max(abs(x - float(y)) for x, y in zip(res['terms'], want_t.mean(dim=0))) <= BOUND
    with pytest.raises(RuntimeError):
        split.feed(a[:1].contiguous(), b[:1].contiguous())                   # result() was taken
    split.reset()
    split.feed(a[:3].contiguous(), b[:3].contiguous())
    with pytest.raises(RuntimeError):
        split.result()                                                      # incomplete
    with pytest.raises(ValueError):
        split.feed(a[:2].contiguous(), b[:2].contiguous())                   # overfeeding
    with pytest.raises(ValueError):
        split.feed(a[:1, :, :16, :16].contiguous(), b[:1, :, :16, :16].contiguous())
    split.feed(a[3:].contiguous(), b[3:].contiguous())
    assert split.result() == res


# ------------------------------------------------------------------------------------------------- the monitor, end to end
@pytest.mark.parametrize('with_ema', [False, True])
def test_monitor_on_a_one_channel_generator(pg, with_ema, deterministic_forward):
    """(``deterministic_forward``: the narrow network's split-K convs commit with atomics otherwise, and the comparison with the
    metric fed directly below is exact.)"""
    torch.manual_seed(7)
    G = pg.Generator((1, 1, 16, 16), latent_size=32, fmap_base=128, fmap_max=32).to('cuda')      # the tiny16c1 configuration
    G.depth = 2
    ema = pg.GeneratorEMA(G, beta=0.5) if with_ema else None
    if with_ema:
        with torch.no_grad():
            G._flat_param.mul_(1.5)                                         # Gs and G now differ
    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=0, G=G, g_ema=ema)
    g = _gen(9)
    drawn = []

    def sample_fn(n):
        drawn.append(torch.randn(n, 32, generator=g))
        return drawn[-1]

    mon = pg.MSSSIMMonitor(sample_fn, num_pairs=8, minibatch=3, msssim_ticks=1)
    mon.register(trainer)
    mon.epoch(1)
    st = trainer.stats
    assert set(st) == {'msssim', 'msssim_std'}
    for name in st:
        v = st[name]['val']
        assert np.isfinite(v) and 0.0 <= v <= 1.0 and st[name]['log_epoch_fields'] == ['{val:.4f}'] and st[name]['log_name'] == name
    assert [z.shape[0] for z in drawn] == [3, 3, 3, 3, 2, 2]
    # the same pairs through the metric directly, from the network the monitor must have used
    net = ema.network() if with_ema else G
    direct = pg.metrics.MultiScaleSSIM(16, 8, num_channels=1)
    for i in range(0, 6, 2):
        a = net.forward(drawn[i].cuda()).clone()
        direct.feed(a, net.forward(drawn[i + 1].cuda()))
    res = direct.result()
    assert st['msssim']['val'] == res['msssim'] and st['msssim_std']['val'] == res['std']
    if with_ema:
        other = pg.metrics.MultiScaleSSIM(16, 8, num_channels=1)
        for i in range(0, 6, 2):
            a = G.forward(drawn[i].cuda()).clone()
            other.feed(a, G.forward(drawn[i + 1].cuda()))
        assert other.result()['msssim'] != res['msssim']


# ------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors(pg):
    ok = torch.zeros(2, 3, 32, 32, device='cuda')
    bad = [(ok.cpu(), ok.cpu()),                                              # host tensors
           (torch.zeros(2, 3, 32, 16, device='cuda'),) * 2,                   # not square
           (torch.zeros(2, 3, 24, 24, device='cuda'),) * 2,                   # not a power of two
           (torch.zeros(2, 3, 8, 8, device='cuda'),) * 2,                     # below 16
           (torch.zeros(2, 2, 32, 32, device='cuda'),) * 2,                   # two channels
           (torch.zeros(2, 4, 32, 32, device='cuda'),) * 2,
           (ok, torch.zeros(3, 3, 32, 32, device='cuda')),                    # mismatched
           (ok, torch.zeros(2, 1, 32, 32, device='cuda')),
           (ok.double(), ok.double()),                                        # not fp32
           (ok, ok.half()),
           (torch.zeros(3, 32, 32, device='cuda'),) * 2]
    for a, b in bad:
        with pytest.raises(ValueError):
            pg.ops.msssim_pairs(a, b)
    with pytest.raises(ValueError):
        pg.ops.msssim_pairs(ok, ok, drange=(1, 1))
    with pytest.raises(ValueError):
        pg.ops.msssim_pairs(ok, ok, scratch=pg.ops.MSSSIMScratch(1, 3, 32, 'cuda'))     # too small a scratch
    with pytest.raises(ValueError):
        pg.ops.msssim_pairs(ok, ok, out=(torch.zeros(2, device='cuda'), torch.zeros(2, 2, device='cuda')))   # fp32 out
    # the C-ABI itself refuses what the wrapper would not send
    part = torch.zeros(64, 2, device='cuda', dtype=torch.float64)
    s = torch.cuda.current_stream().cuda_stream
    call = pg._lib.load().pg_msssim_scale
    img = torch.zeros(1, 1, 16, 16, device='cuda')
    assert call(img.data_ptr(), img.data_ptr(), None, None, part.data_ptr(), 1, 24, 2, -1.0, 1.0, s) == -1
    assert call(img.data_ptr(), img.data_ptr(), None, None, part.data_ptr(), 1, 8, 2, -1.0, 1.0, s) == -1
    assert call(img.data_ptr(), img.data_ptr(), img.data_ptr(), img.data_ptr(), part.data_ptr(), 1, 16, 2, -1.0, 1.0, s) == -1
    assert call(img.data_ptr(), img.data_ptr(), None, None, part.data_ptr(), 1, 16, 2, 1.0, 1.0, s) == -1
    assert call(img.data_ptr(), None, None, None, part.data_ptr(), 1, 16, 2, -1.0, 1.0, s) == -1
