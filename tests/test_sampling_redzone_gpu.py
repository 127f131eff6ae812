"""Every entry point of include/pggan_hip_sampling.h between guard bands (tests/redzone.py, docs/experiments_redzone.md) at its ragged
shapes: N = 3 (no multiple of the 4 images a 4x4 tile holds), Cout = 8 and 40 (half a cout tile, two and a half), H = 4, Cin = 24 (a
partial chunk); n = 1, 7 and 4099 for the cast.  Inputs sit between bands of 0x7F7F (bf16: 3.4e38) or NaN (fp32): a load from outside
that reaches the result breaks the comparison with tests/sampling_ref.py.  Outputs are created through the allocator proxy, filled
with the sentinel: no band is touched, no input modified, every output element written."""
import numpy as np
import pytest
import torch

import sampling_ref as ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops, smp = pg.ops, pg.sampling
EPS = 1e-8


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    proxy = r.proxy(helpers=(ops._empty, ops.Arena.take))
    monkeypatch.setattr(ops, 'torch', proxy)
    monkeypatch.setattr(smp, 'torch', proxy)
    yield r
    r.forget()


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


def bf16(t64):
    return t64.float().to(torch.bfloat16)


def close(got, want, e32):
    got = got.detach().float().cpu().double()
    return bool(((got - want).abs() <= ref.contract_bound(want, e32)).all())


@pytest.mark.parametrize('n', [1, 7, 4099])
def test_cast_inside_guard_bands(rz, n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    x_d = rz.guard(x, name='x')
    assert x_d.data_ptr() % 32 == 16
    got = smp.cast_bf16(x_d)
    chk(rz)
    assert got.data_ptr() % 32 == 16 and torch.equal(got.cpu().view(torch.int16), x.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize('N,H,cin,cout,ups', [(3, 4, 8, 8, False), (3, 4, 24, 40, False), (3, 8, 16, 8, True), (1, 16, 40, 40, True)])
def test_conv_and_pixelnorm_inside_guard_bands(rz, N, H, cin, cout, ups):
    g = torch.Generator().manual_seed(cin * 100 + cout)
    Hin = H // 2 if ups else H
    a = ref.rne_bf16(torch.randn(N, Hin, Hin, cin, generator=g, dtype=torch.float64))
    wb = ref.rne_bf16(torch.randn(3, 3, cout, cin, generator=g, dtype=torch.float64))
    bias = 0.1 * torch.randn(cout, generator=g)
    c = float(np.sqrt(2.0 / (9 * cin)))
    a_d, w_d, b_d = rz.guard(bf16(a), name='x'), rz.guard(bf16(wb), name='w'), rz.guard(bias, name='bias')
    assert a_d.data_ptr() % 32 == 16 and w_d.data_ptr() % 32 == 16
    for pn in (False, True):
        want = ref.layer_ref(a, wb, bias.double(), c, 0.2, EPS, ups=ups, pn=pn, rounded=False)
        e32 = float((ref.layer_ref(a.float(), wb.float(), bias, c, 0.2, EPS, ups=ups, pn=pn, rounded=False).double() - want).abs().max())
        y = smp.conv3_bf16(a_d, w_d, b_d, N, Hin, Hin, c, 0.2, EPS, ups=ups, pixelnorm=pn)
        chk(rz)                                                # bands intact, inputs unchanged, every output element written
        assert y.data_ptr() % 32 == 16 and close(y, want, e32)
    y32 = smp.conv3_bf16(a_d, w_d, b_d, N, Hin, Hin, c, 0.2, EPS, ups=ups, out_f32=True)
    chk(rz, keep_outputs=True)                                 # (y32 stays a guarded tensor: it is the next launch's input)
    y = smp.pixelnorm_bf16(y32, EPS)
    chk(rz)
    assert close(y, want, e32)
    y = smp.conv3_bf16(a_d, w_d, None, N, Hin, Hin, c, 0.0, EPS, ups=ups)            # no bias, ReLU
    chk(rz)
    assert close(y, ref.layer_ref(a, wb, None, c, 0.0, EPS, ups=ups, pn=False, rounded=False), e32)


@pytest.mark.parametrize('C,cin,pcin', [(3, 8, 16), (1, 40, 40), (2, 24, 8)])
def test_torgb_inside_guard_bands(rz, C, cin, pcin):
    N, H = 3, 4
    g = torch.Generator().manual_seed(C * 10 + cin)
    x = ref.rne_bf16(torch.randn(N, H, H, cin, generator=g, dtype=torch.float64))
    px = ref.rne_bf16(torch.randn(N, H // 2, H // 2, pcin, generator=g, dtype=torch.float64))
    w, b, pw, pb = torch.randn(C, cin, generator=g), torch.randn(C, generator=g), torch.randn(C, pcin, generator=g), torch.randn(C, generator=g)
    x_d, px_d = rz.guard(bf16(x), name='x'), rz.guard(bf16(px), name='prev')
    w_d, b_d, pw_d, pb_d = (rz.guard(t, name=n) for t, n in ((w, 'w'), (b, 'bias'), (pw, 'prev_w'), (pb, 'prev_bias')))
    got = smp.torgb_bf16(x_d, w_d, b_d, N, C, H, H, 0.3)
    chk(rz)
    want = ref.torgb_ref(x, w.double(), b.double(), 0.3)
    assert got.data_ptr() % 32 == 16 and float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    got = smp.torgb_bf16(x_d, w_d, b_d, N, C, H, H, 0.3, out_mul=0.25, prev=px_d, prev_w=pw_d, prev_bias=pb_d, prev_scale=0.7, prev_mul=0.75)
    chk(rz)
    want = ref.torgb_ref(x, w.double(), b.double(), 0.3, 0.25, px, pw.double(), pb.double(), 0.7, 0.75)
    assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_sampler_forward_inside_guard_bands(rz):
    """The whole pass, its own allocations (the bf16 twin, block 0's fp32 output, every activation, the image) between bands."""
    torch.manual_seed(5)
    G = pg.Generator((1, 3, 16, 16), fmap_base=128, fmap_max=32, latent_size=32).to('cuda')        # 32, 32, 16 channels
    G.depth, G.alpha = 2, 0.5
    z = torch.randn(3, 32, generator=torch.Generator().manual_seed(6))
    z_d = rz.guard(z, name='z')
    img, acts = pg.Sampler(G).forward(z_d, return_activations=True)
    chk(rz)
    want = ref.generator_ref(G, z, rounded=True)
    move = float((img.cpu().double() - want).norm() / want.norm())
    print('image against the CPU contract: relative L2 %.3e' % move)
    assert tuple(img.shape) == (3, 3, 16, 16) and len(acts) == 6 and move < 2e-2
