"""TEST INFRASTRUCTURE: the contract of the bf16 sampling path (include/pggan_hip_sampling.h) restated in torch on the
CPU.  Everything here is plain torch in the dtype of its operands -- fp64 for the references, float32 where a test wants the error of
a float32 evaluation of the same formula (``e32``).  The rounding points are the contract's and there are no others:

  rne_bf16(v)       round to nearest even to bf16, NaN stays NaN; the result is returned in v's dtype
  layer_ref         y = rne(PN(lrelu(c * conv3x3(a, wb) + b))), nearest x2 upsampling of ``a`` first where the layer has it
  generator_ref     the whole network: weights rounded once, block 0's c1 evaluated unrounded and rounded once, every 3x3 layer by
                    layer_ref, toRGB and the fade-in blend unrounded.  ``rounded=False`` drops every rounding: the reference network."""
import torch
import torch.nn.functional as F

BF16_MANT = 8                    # significand bits, the implicit one included
BF16_EMIN = -125                 # frexp exponent of the smallest normal, 2^-126 = 0.5 * 2^-125
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127


def _ulp(x):
    """Spacing of the bf16 grid around |x| (fp64; the subnormal spacing below the smallest normal; 2^-133 at zero)."""
    _, e = torch.frexp(x.abs().double())
    e = torch.where(torch.isfinite(x.double()) & (x != 0), e, torch.full_like(e, BF16_EMIN))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e.clamp(min=BF16_EMIN) - BF16_MANT)


def half_ulp_bf16(x):
    """Half the bf16 spacing at |x|: the most a correctly rounded bf16 value may differ from x."""
    return 0.5 * _ulp(x)


def rne_bf16(x):
    """Round to nearest even onto the bf16 grid (subnormals included, overflow to infinity, NaN and infinities as they are)."""
    x64 = x.double()
    u = _ulp(x64)
    y = torch.round(x64 / u) * u                                       # torch.round: half to even; x64 / u is exact (u a power of two)
    y = torch.where(y.abs() > BF16_MAX, torch.sign(y) * float('inf'), y)
    y = torch.where(torch.isfinite(x64), y, x64)
    return y.to(x.dtype)


def bf16_bits(x):
    """int32 bit patterns (0 .. 65535) of a tensor of bf16-representable values."""
    return (x.float().contiguous().view(torch.int32) >> 16) & 0xFFFF


def special_values():
    """Ties to even both ways, +-0, fp32 denormals, values that round up into the next binade, +-inf, the largest finite, NaN."""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,        # 1 + 2^-8 (tie, down to even), 1 + 3 * 2^-8 (tie, up to even)
            0x3F808001, 0x3F807FFF,                                # just above / below a tie
            0x00000000, 0x80000000,                                # +-0
            0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x0000FFFF,       # fp32 denormals (ties among them)
            0x3FFFFFFF, 0x3FFF8000, 0xBFFFC000, 0x007FFFFF,        # round up into the next binade
            0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000,       # inf, largest finite (overflows), largest bf16
            0x7FC00000, 0x7F800001, 0xFFC12345]                    # NaN
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def pixelnorm(v, eps=1e-8, dim=1):
    return v / torch.sqrt(torch.mean(v * v, dim, keepdim=True) + eps)


def layer_ref(a, wb, bias, c, slope, eps=1e-8, ups=False, pn=True, rounded=True):
    """One 3x3 pad-1 layer.  a [N,Hin,Win,Cin] (NHWC), wb [3,3,Cout,Cin] (the stored layout), bias [Cout] or None, all of one dtype ->
    [N,H,W,Cout] in that dtype; ``rounded=False`` returns the value before the one rounding."""
    x = a.permute(0, 3, 1, 2)
    if ups:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    v = c * F.conv2d(x, wb.permute(2, 3, 0, 1), None, 1, 1)
    if bias is not None:
        v = v + bias.view(1, -1, 1, 1)
    v = torch.where(v > 0, v, v * slope)
    if pn:
        v = pixelnorm(v, eps)
    v = v.permute(0, 2, 3, 1).contiguous()
    return rne_bf16(v) if rounded else v


def torgb_ref(x, w, bias, c, out_mul=1.0, prev=None, prev_w=None, prev_bias=None, prev_c=1.0, prev_mul=0.0):
    """x [N,H,W,Cin], w [C,Cin] -> [N,C,H,W] = out_mul (c w.x + bias) + prev_mul (prev_c prev_w.prev + prev_bias), prev at (h >> 1, w >> 1)."""
    img = out_mul * (c * torch.einsum('nhwk,ck->nchw', x, w) + bias.view(1, -1, 1, 1))
    if prev is not None:
        p = prev_c * torch.einsum('nhwk,ck->nchw', prev, prev_w) + prev_bias.view(1, -1, 1, 1)
        img = prev_mul * p.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) + img
    return img


def conv3_layers(G):
    out = [('block0.c2', G.block0.c2)]
    for i, blk in enumerate(G.blocks):
        out += [('blocks.%d.c1' % i, blk.c1), ('blocks.%d.c2' % i, blk.c2)]
    return out


def generator_ref(G, z, rounded=True, depth=None, alpha=None, return_activations=False):
    """The contract on a ``pg.Generator`` (any device; evaluated on the CPU in fp64).  z [N, latent].  Returns the fp64 NCHW image, and
    with ``return_activations`` the list of layer outputs (NHWC fp64) in evaluation order."""
    depth = int(G.depth) if depth is None else depth
    alpha = float(G.alpha) if alpha is None else alpha
    d = lambda t: t.detach().cpu().double()
    r = rne_bf16 if rounded else (lambda t: t)
    h = d(z)
    if G.normalize_latents:
        h = pixelnorm(h, G.eps)
    c1 = G.block0.c1                                                    # 4x4 pad 3 on the 1x1 latent: fp32 weights, rounded once
    v = c1.c * F.conv2d(h[:, :, None, None], d(c1.conv.weight)[..., :c1.ch_in].permute(2, 3, 0, 1), None, 1, 3) + d(c1.conv.bias).view(1, -1, 1, 1)
    v = torch.where(v > 0, v, v * c1.slope)
    if c1.pixelnorm:
        v = pixelnorm(v, c1.eps)
    h = r(v.permute(0, 2, 3, 1).contiguous())
    acts = [h]

    def layer(x, lay, ups=False):
        y = layer_ref(x, r(d(lay.conv.weight)), d(lay.conv.bias), lay.c, lay.slope, lay.eps, ups=ups, pn=lay.pixelnorm, rounded=rounded)
        acts.append(y)
        return y

    h = layer(h, G.block0.c2)
    hprev = None
    for i in range(depth):
        hprev = h
        h = layer(layer(h, G.blocks[i].c1, ups=True), G.blocks[i].c2)
    t = G.blocks[depth - 1].toRGB if depth > 0 else G.block0.toRGB
    if depth > 0 and alpha < 1.0:
        pt = G.blocks[depth - 2].toRGB if depth > 1 else G.block0.toRGB
        img = torgb_ref(h, d(t.conv.weight), d(t.conv.bias), t.c, alpha, hprev, d(pt.conv.weight), d(pt.conv.bias), pt.c, 1.0 - alpha)
    else:
        img = torgb_ref(h, d(t.conv.weight), d(t.conv.bias), t.c)
    return (img, acts) if return_activations else img


def contract_bound(y_ref, e32, out_f32=False):
    """The per-element bound of the conv contract: half a bf16 ulp at |y_ref| + 3 e32, plus 3 e32 (e32: the largest error of a float32
    evaluation of the same layer against fp64 -- two fp32 summation orders differ from each other by as much as either does from fp64)."""
    if out_f32:
        return torch.full_like(y_ref, 3.0 * e32)
    return half_ulp_bf16(y_ref.abs() + 3.0 * e32) + 3.0 * e32
