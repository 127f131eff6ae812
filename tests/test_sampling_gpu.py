"""GPU tier of the bf16 sampling path (csrc/sampling.hip, pggan-pytorch_amd/sampling.py) against tests/sampling_ref.py.

The conv contract, per element: y_ref is the layer in fp64 from the kernel's OWN bf16 inputs, e32 the largest error against that fp64
of a torch float32 CPU evaluation of the same layer on the same operands, and

    |y - y_ref|  <=  half_ulp_bf16(|y_ref| + 3 e32) + 3 e32                       (3 e32 alone where the output is fp32)

The 3x on a float32 reference's own error is the project's adjudicator rule: two fp32 summation orders disagree with each other by as
much as either disagrees with fp64.  Each case asserts that 3 e32 is below 1/100 of its median half-ulp, so the bf16 term decides.
Every comparison prints its measured maximum (as a ratio to the bound) before it asserts."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampling_ref as ref

import pggan_amd as pg

pytestmark = pytest.mark.gpu
smp = pg.sampling
DEV = 'cuda'


def bf16_dev(t64):
    """A tensor of bf16-representable values -> the bf16 device tensor holding exactly them."""
    return t64.float().to(torch.bfloat16).to(DEV).contiguous()


def host64(t):
    return t.detach().float().cpu().double()


def held(name, got, want, bound):
    """Print the largest |got - want| / bound, then assert that it is at most 1 (NaN anywhere fails)."""
    got, want = host64(got), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ratio = (got - want).abs() / bound
    worst = float(ratio.max())
    print('%s: largest error / bound = %.4f  (largest error %.3e)' % (name, worst, float((got - want).abs().max())))
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, name


# ------------------------------------------------------------------------------------------------ cast
@pytest.mark.parametrize('n', [1, 7, 8, 4099])
def test_cast_is_torch_conversion_bitwise(n):
    g = torch.Generator().manual_seed(n)
    pool = torch.cat([ref.special_values(), torch.randn(4099, generator=g) * torch.tensor([1.0, 1e-38, 1e-41, 1e37]).repeat(1025)[:4099]])
    chunks = [pool[i:i + n] for i in range(0, len(ref.special_values()) if n < 4099 else 1, n)]
    for x in chunks:
        if x.numel() < n:
            x = torch.cat([x, pool[:n - x.numel()]])
        got = smp.cast_bf16(x.to(DEV)).cpu()
        want = x.to(torch.bfloat16)
        nan = torch.isnan(x)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (n,)
        assert bool(torch.isnan(got[nan].float()).all())
        assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))
    print('cast n = %d: %d launches bit-identical to torch' % (n, len(chunks)))


# ------------------------------------------------------------------------------------------------ conv contract
UPS, PN = 'UPSAMPLE', 'PIXELNORM'
SHAPES = [(3, 4, 8, 8), (1, 4, 512, 512), (2, 8, 16, 8, UPS), (2, 16, 24, 40), (1, 32, 64, 32, UPS), (1, 64, 8, 8),
          (3, 16, 512, 512, PN)]
EPS = 1e-8


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """Operands of a shape and its two CPU evaluations up to the bias (shared by every route and slope; never modified)."""
    N, H, cin, cout = shape[:4]
    ups = UPS in shape
    g = torch.Generator().manual_seed(1000 * cin + cout + H)
    Hin = H // 2 if ups else H
    a = ref.rne_bf16(torch.randn(N, Hin, Hin, cin, generator=g, dtype=torch.float64))
    wb = ref.rne_bf16(torch.randn(3, 3, cout, cin, generator=g, dtype=torch.float64))
    bias = (0.1 * torch.randn(cout, generator=g)).double()
    c = float(np.sqrt(2.0 / (9 * cin)))

    def pre(dtype):
        # The sum runs over 64-channel blocks.  In fp64 that changes nothing worth naming; in float32 it is still a torch float32 CPU
        # evaluation of the layer, with the error of a blocked sum: torch's one-call CPU conv measured e32 = 1.3e-5 at (3, 16, 512, 512),
        # K = 4608 -- above the criterion's own condition (3 e32 < median half-ulp / 100), where the blocked sum gives 1e-6.  A smaller
        # e32 makes every bound below tighter, never wider.
        x = a.to(dtype).permute(0, 3, 1, 2)
        if ups:
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        w = wb.to(dtype).permute(2, 3, 0, 1)
        s = sum(F.conv2d(x[:, i:i + 64], w[:, i:i + 64], None, 1, 1) for i in range(0, cin, 64))
        return torch.tensor(c, dtype=dtype) * s + bias.to(dtype).view(1, -1, 1, 1)
    return dict(N=N, H=H, Hin=Hin, cin=cin, cout=cout, ups=ups, a=a, wb=wb, bias=bias, c=c, pre64=pre(torch.float64), pre32=pre(torch.float32),
                a_d=bf16_dev(a), wb_d=bf16_dev(wb), bias_d=bias.float().to(DEV))


def epilogue(pre, slope, pn):
    v = torch.where(pre > 0, pre, pre * slope)
    if pn:
        v = ref.pixelnorm(v, EPS)
    return v.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('slope', [0.2, 0.0])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_conv_contract(shape, slope):
    k = conv_case(shape)
    call = lambda **kw: smp.conv3_bf16(k['a_d'], k['wb_d'], k['bias_d'], k['N'], k['Hin'], k['Hin'], k['c'], slope, EPS, ups=k['ups'], **kw)
    for pn in (False, True):
        y_ref = epilogue(k['pre64'], slope, pn)
        e32 = float((epilogue(k['pre32'], slope, pn).double() - y_ref).abs().max())
        median_half_ulp = float(ref.half_ulp_bf16(y_ref[y_ref != 0]).median())
        print('%s slope %g pn %d: e32 = %.3e, median half-ulp = %.3e' % (shape, slope, pn, e32, median_half_ulp))
        assert 3 * e32 < median_half_ulp / 100                          # the condition of the criterion: the bf16 term decides
        tag = '%s slope %g %s' % ('x'.join(str(v) for v in shape), slope, 'pn' if pn else 'plain')
        if pn and k['cout'] > smp.PIXELNORM_MAX_COUT:
            with pytest.raises(pg.ops.Unsupported):                      # too wide for one wave: the caller takes the two-launch route
                call(pixelnorm=True)
        else:
            y = call(pixelnorm=pn)
            assert y.dtype == torch.bfloat16
            held(tag + ' fused', y, y_ref, ref.contract_bound(y_ref, e32))
        if not pn:
            y32 = call(out_f32=True)
            assert y32.dtype == torch.float32
            held(tag + ' fp32 out', y32, y_ref, ref.contract_bound(y_ref, e32, out_f32=True))
        else:
            y = smp.pixelnorm_bf16(call(out_f32=True), EPS)
            assert y.dtype == torch.bfloat16
            held(tag + ' fp32 out + pixelnorm', y, y_ref, ref.contract_bound(y_ref, e32))


# The pixel tile of a workgroup grows from 64 to 128, 256 and 512 pixels once that still leaves 512 workgroups, and a single-chunk
# layer with more than 2048 tiles walks them with its weights kept in LDS: the smallest shapes that take each of those paths
# (cout fragments x pixel fragments per wave in the comment; the shapes above all run 64-pixel tiles).
LARGE_TILES = [(2, 1024, 8, 8, PN),            # 1 x 8, 4096 tiles on 2048 workgroups
               (2, 256, 8, 64),                # 4 x 4
               (1, 256, 8, 128, PN),           # 8 x 2
               (1, 256, 40, 64, UPS)]          # 4 x 2, two chunks (32 + 8 channels)


@pytest.mark.parametrize('shape', LARGE_TILES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_conv_contract_large_tiles(shape):
    k = conv_case(shape)
    pn = PN in shape
    y_ref = epilogue(k['pre64'], 0.2, pn)
    e32 = float((epilogue(k['pre32'], 0.2, pn).double() - y_ref).abs().max())
    assert 3 * e32 < float(ref.half_ulp_bf16(y_ref[y_ref != 0]).median()) / 100
    y = smp.conv3_bf16(k['a_d'], k['wb_d'], k['bias_d'], k['N'], k['Hin'], k['Hin'], k['c'], 0.2, EPS, ups=k['ups'], pixelnorm=pn)
    held('x'.join(str(v) for v in shape) + ' (e32 %.2e)' % e32, y, y_ref, ref.contract_bound(y_ref, e32))
    if not pn:
        y = smp.conv3_bf16(k['a_d'], k['wb_d'], k['bias_d'], k['N'], k['Hin'], k['Hin'], k['c'], 0.2, EPS, ups=k['ups'], out_f32=True)
        held('x'.join(str(v) for v in shape) + ' fp32 out', y, y_ref, ref.contract_bound(y_ref, e32, out_f32=True))


def test_conv_refuses_what_it_does_not_take():
    x = torch.zeros(1, 4, 4, 12, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(3, 3, 8, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):
        smp.conv3_bf16(x, w, None, 1, 4, 4, 1.0, 0.2)
    x = torch.zeros(1, 6, 6, 8, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(3, 3, 8, 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(pg.ops.Unsupported):
        smp.conv3_bf16(x, w, None, 1, 6, 6, 1.0, 0.2)
    with pytest.raises(ValueError):
        smp.conv3_bf16(x.float(), w, None, 1, 6, 6, 1.0, 0.2)


# ------------------------------------------------------------------------------------------------ toRGB
@pytest.mark.parametrize('alpha', [1.0, 0.5])
@pytest.mark.parametrize('H', [4, 16])
@pytest.mark.parametrize('cin', [8, 40, 512])
@pytest.mark.parametrize('C', [1, 2, 3])
def test_torgb(C, cin, H, alpha):
    N = 3
    g = torch.Generator().manual_seed(C * 1000 + cin + H)
    pcin = 16 if cin == 8 else cin
    x = ref.rne_bf16(torch.randn(N, H, H, cin, generator=g, dtype=torch.float64))
    w, b = torch.randn(C, cin, generator=g), 0.1 * torch.randn(C, generator=g)
    px = ref.rne_bf16(torch.randn(N, H // 2, H // 2, pcin, generator=g, dtype=torch.float64))
    pw, pb = torch.randn(C, pcin, generator=g), 0.1 * torch.randn(C, generator=g)
    c, pc = float(np.sqrt(1.0 / cin)), float(np.sqrt(1.0 / pcin))
    if alpha < 1.0:
        evaluate = lambda t: ref.torgb_ref(x.to(t), w.to(t), b.to(t), c, alpha, px.to(t), pw.to(t), pb.to(t), pc, 1.0 - alpha)
        got = smp.torgb_bf16(bf16_dev(x), w.to(DEV), b.to(DEV), N, C, H, H, c, out_mul=alpha, prev=bf16_dev(px), prev_w=pw.to(DEV),
                             prev_bias=pb.to(DEV), prev_scale=pc, prev_mul=1.0 - alpha)
    else:
        evaluate = lambda t: ref.torgb_ref(x.to(t), w.to(t), b.to(t), c)
        got = smp.torgb_bf16(bf16_dev(x), w.to(DEV), b.to(DEV), N, C, H, H, c)
    want = evaluate(torch.float64)
    e32 = float((evaluate(torch.float32).double() - want).abs().max())
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, C, H, H)
    held('toRGB C %d cin %d H %d alpha %g (e32 %.3e)' % (C, cin, H, alpha, e32), got, want, torch.full_like(want, 3 * e32))


# ------------------------------------------------------------------------------------------------ the network
@functools.lru_cache(maxsize=None)
def chain_net():
    torch.manual_seed(11)
    G = pg.Generator((1, 3, 32, 32), fmap_base=512, fmap_max=64, latent_size=64)
    with torch.no_grad():
        for p in G.parameters():                                         # (biases start at zero: give them work)
            if p.dim() == 1:
                p.normal_(0.0, 0.1)
    G.to(DEV)
    z = torch.randn(3, 64, generator=torch.Generator().manual_seed(12))
    return G, z


def _stage(G, depth, alpha):
    G.depth, G.alpha = depth, alpha
    return G


@pytest.mark.parametrize('depth,alpha', [(0, 1.0), (1, 0.5), (2, 0.5), (3, 0.5), (3, 1.0)])
def test_chain_every_layer_from_the_kernels_own_input(depth, alpha):
    G, z = chain_net()
    _stage(G, depth, alpha)
    img, acts = pg.Sampler(G).forward(z.to(DEV), return_activations=True)
    assert len(acts) == 2 + 2 * depth and all(a.dtype == torch.bfloat16 for a in acts)
    d = lambda t: t.detach().cpu().double()
    # block 0, c1: the fp32 path's result, rounded once
    c1 = G.block0.c1

    def first(t):
        h = ref.pixelnorm(z.to(t), G.eps)
        v = c1.c * F.conv2d(h[:, :, None, None], d(c1.conv.weight).to(t).permute(2, 3, 0, 1), None, 1, 3) + d(c1.conv.bias).to(t).view(1, -1, 1, 1)
        return ref.pixelnorm(torch.where(v > 0, v, v * c1.slope), c1.eps).permute(0, 2, 3, 1).contiguous()
    y_ref = first(torch.float64)
    e32 = float((first(torch.float32).double() - y_ref).abs().max())
    held('depth %d block0.c1 (e32 %.2e)' % (depth, e32), acts[0], y_ref, ref.contract_bound(y_ref, e32))
    # every 3x3 layer from the kernel's own previous activation
    layers = ref.conv3_layers(G)[:1 + 2 * depth]
    for i, (name, lay) in enumerate(layers):
        ups = name.endswith('.c1') and name != 'block0.c1'
        a, wb, b = host64(acts[i]), ref.rne_bf16(d(lay.conv.weight)), d(lay.conv.bias)
        y_ref = ref.layer_ref(a, wb, b, lay.c, lay.slope, lay.eps, ups=ups, pn=lay.pixelnorm, rounded=False)
        y32 = ref.layer_ref(a.float(), wb.float(), b.float(), lay.c, lay.slope, lay.eps, ups=ups, pn=lay.pixelnorm, rounded=False)
        e32 = float((y32.double() - y_ref).abs().max())
        assert 3 * e32 < float(ref.half_ulp_bf16(y_ref).median()) / 100
        held('depth %d %s (e32 %.2e)' % (depth, name, e32), acts[i + 1], y_ref, ref.contract_bound(y_ref, e32))
    # toRGB and the blend from the kernel's own activations
    t = G.blocks[depth - 1].toRGB if depth else G.block0.toRGB
    if depth and alpha < 1.0:
        pt = G.blocks[depth - 2].toRGB if depth > 1 else G.block0.toRGB
        ev = lambda ty: ref.torgb_ref(host64(acts[-1]).to(ty), d(t.conv.weight).to(ty), d(t.conv.bias).to(ty), t.c, alpha, host64(acts[-3]).to(ty),
                                      d(pt.conv.weight).to(ty), d(pt.conv.bias).to(ty), pt.c, 1.0 - alpha)
    else:
        ev = lambda ty: ref.torgb_ref(host64(acts[-1]).to(ty), d(t.conv.weight).to(ty), d(t.conv.bias).to(ty), t.c)
    want = ev(torch.float64)
    e32 = float((ev(torch.float32).double() - want).abs().max())
    held('depth %d image (e32 %.2e)' % (depth, e32), img, want, torch.full_like(want, 3 * e32))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_end_to_end_against_the_fp32_generator(alpha):
    """The image moves no further from G.forward's than 3x what the CPU reference says bf16 moves this network (ties that fall
    differently decorrelate single pixels, hence the margin; the measured ratio is in docs/experiments_sampling.md)."""
    G, _ = chain_net()
    _stage(G, 3, alpha)
    z = torch.randn(8, 64, generator=torch.Generator().manual_seed(13))
    ref_move = rel_l2(ref.generator_ref(G, z, rounded=True), ref.generator_ref(G, z, rounded=False))
    fp32 = G.forward(z.to(DEV)).cpu()
    got = pg.sampler_for(G)(z.to(DEV)).cpu()
    assert got.dtype == torch.float32 and got.shape == fp32.shape
    move = rel_l2(got, fp32)
    print('alpha %g: bf16 image against fp32 image, relative L2 %.4e; the reference moves %.4e; ratio %.3f; max |diff| %.3e'
          % (alpha, move, ref_move, move / ref_move, float((got - fp32).abs().max())))
    assert 0.0 < move <= 3.0 * ref_move


def test_reproducible_and_follows_the_parameters():
    torch.manual_seed(21)
    G = pg.Generator((1, 3, 32, 32), fmap_base=512, fmap_max=64, latent_size=64).to(DEV)
    G.depth, G.alpha = 3, 0.5
    z = torch.randn(4, 64, device=DEV)
    s = pg.sampler_for(G)
    a = s(z)
    assert torch.equal(a, s(z))                                          # two calls, equal bits
    with torch.no_grad():
        G._flat_param.mul_(1.01)
    G.mark_params_changed()
    b = s(z)
    assert not torch.equal(a, b) and torch.equal(b, pg.Sampler(G)(z))    # the twin was refreshed: a fresh sampler agrees bit for bit
    sd = {k: v.clone() * 0.97 for k, v in G.state_dict().items()}
    G.load_state_dict(sd)                                                # torch-side update: the _sync_version route
    c = s(z)
    assert not torch.equal(b, c) and torch.equal(c, pg.Sampler(G)(z))
    G.depth, G.alpha = 1, 1.0                                            # depth and alpha are read at call time
    assert tuple(s(z).shape) == (4, 3, 8, 8)


def test_sampler_of_the_smoothed_generator_follows_update():
    torch.manual_seed(22)
    G = pg.Generator((1, 3, 32, 32), fmap_base=512, fmap_max=64, latent_size=64).to(DEV)
    G.depth, G.alpha = 2, 1.0
    ema = pg.GeneratorEMA(G, beta=0.5)
    z = torch.randn(2, 64, device=DEV)
    s = pg.sampler_for(ema.network())
    a = s(z)
    assert tuple(a.shape) == (2, 3, 16, 16) and torch.equal(a, pg.sampler_for(G)(z))       # the average starts as a copy of G
    with torch.no_grad():
        G._flat_param.mul_(1.1)
    G.mark_params_changed()
    ema.update(16)
    assert pg.sampler_for(ema.network()) is s
    b = s(z)
    assert not torch.equal(a, b) and torch.equal(b, pg.Sampler(ema.network())(z))
    assert not torch.equal(b, pg.sampler_for(G)(z))


class _StubTrainer(object):
    parallel = None
    g_ema = None
    cur_nimg = 0

    def __init__(self, G):
        self.G, self.stats = G, {}


def test_msssim_monitor_in_bf16_measures_the_samplers_images():
    G, _ = chain_net()
    _stage(G, 3, 1.0)

    def latents():
        g = torch.Generator().manual_seed(31)
        return lambda n: torch.randn(n, 64, generator=g)
    mon = pg.MSSSIMMonitor(latents(), num_pairs=4, minibatch=2, precision='bf16')
    tr = _StubTrainer(G)
    mon.register(tr)
    mon.epoch(0)
    fn, s = latents(), pg.sampler_for(G)
    metric = pg.metrics.MultiScaleSSIM(32, 4, num_channels=3)
    for _ in range(2):
        a = s(fn(2).to(DEV))
        metric.feed(a, s(fn(2).to(DEV)))
    want = metric.result()
    print('msssim through the monitor %.6f, fed by hand %.6f' % (tr.stats['msssim']['val'], want['msssim']))
    assert tr.stats['msssim']['val'] == want['msssim'] and tr.stats['msssim_std']['val'] == want['std']
    fp32 = pg.MSSSIMMonitor(latents(), num_pairs=4, minibatch=2)
    fp32.register(tr)
    fp32.epoch(0)
    print('msssim in fp32 %.6f' % tr.stats['msssim']['val'])
