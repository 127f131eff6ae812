"""Forward-only generator in bf16 (include/pggan_hip_sampling.h, csrc/sampling.hip; DESIGN.md §7 "bf16 sampling path").

Everything that only LOOKS at the generator -- sample grids, ``DeviceSoundSaver``, the four metric monitors -- can evaluate it on the
bf16 matrix cores with half-width activations: ``Sampler(net)(z)`` takes fp32 latents and returns the fp32 NCHW image ``net.forward(z)``
returns, so no consumer changes.  Opt-in (``precision='bf16'`` of the output plugins and ``utils.output_samples``); the training step
and the default of every consumer stay fp32.  The contract, whatever the kernels fuse -- rne = round to nearest even, NaN stays NaN:

  1. weights      wb = rne(w) of every 3x3 weight in its stored layout; the equalized-lr constant c is applied in fp32 in the epilogue,
                  biases and toRGB weights stay fp32.  ONE cast launch over the flat parameter buffer makes a bf16 twin with the same
                  offsets (padding and biases are cast too and never read), refreshed when ``net._param_version`` has moved or the
                  buffer was replaced.
  2. block 0, c1  (4x4 on the 1x1 latent) runs on the fp32 path and is rounded once, y1 = rne(fp32 result).
  3. 3x3 layers   y = rne(PN(lrelu(c * sum_k a_k wb_k + b))): bf16 input (nearest x2 upsampling in the gather), fp32 accumulation on
                  the MFMA, fp32 epilogue, one rounding after PixelNorm -- in one launch up to ``PIXELNORM_MAX_COUT`` output channels,
                  through an fp32 scratch and ``pixelnorm_bf16`` above that (the same formula binds the result).
  4. toRGB        and the fade-in blend with the previous stage's toRGB read bf16 activations, compute in fp32 with fp32 weights and
                  write the fp32 image.

No atomics: two calls give the same bits (block 0's c1 included where the latent size and its width are multiples of 16, the skinny
GEMM of csrc/conv_k4.hip; other widths go through the direct conv, whose small maps commit K slices with atomics).  There is no CPU
path.  Measured on an MI355X, 16 images per call (docs/experiments_sampling.md): 2.90 ms against ``G.forward``'s 2.44 ms at the 1024x1024
stage (0.84x), 0.98 - 1.05x at 128x128 .. 512x512, 0.44 - 0.81x below: this first bf16 kernel does not yet beat the fp32 Winograd path;
the images differ from the fp32 ones by about 1 % relative L2."""
import weakref

import torch

from . import _lib, engine, ops

_C = _lib.SAMPLING_CONSTANTS
FLAG_UPSAMPLE, FLAG_PIXELNORM, FLAG_OUT_F32 = _C['PG_SMP_UPSAMPLE'], _C['PG_SMP_PIXELNORM'], _C['PG_SMP_OUT_F32']
PIXELNORM_MAX_COUT = _C['PG_SMP_PIXELNORM_MAX_COUT']
TORGB_MAX_C = _C['PG_SMP_TORGB_MAX_C']
PRECISIONS = ('fp32', 'bf16')
_BF16, _F32 = torch.bfloat16, torch.float32


def _ptr(t, dtype, what):
    """Device pointer of a checked tensor (None -> NULL)."""
    if t is None:
        return None
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype is not dtype or not t.is_contiguous():
        raise ValueError('%s: expected a contiguous %s device tensor, got %s %s on %s'
                         % (what, dtype, tuple(getattr(t, 'shape', ())), getattr(t, 'dtype', type(t)), getattr(t, 'device', None)))
    return t.data_ptr()


# ------------------------------------------------------------------------------------ the four entry points
def cast_bf16(x, out=None):
    """fp32 tensor -> bf16 tensor of its shape, round to nearest even (NaN stays NaN).  One launch."""
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=_BF16)
    if out.numel() != x.numel():
        raise ValueError('cast_bf16: %d elements into %d' % (x.numel(), out.numel()))
    _lib.call('pg_smp_cast_bf16', _ptr(x, _F32, 'x'), _ptr(out, _BF16, 'out'), x.numel(), ops._stream())
    return out


def conv3_bf16(x, w, bias, N, Hin, Win, scale, slope, eps=1e-8, ups=False, pixelnorm=False, out_f32=False):
    """The 3x3 layer of the contract.  x [N,Hin,Win,Cin] bf16, w [3,3,Cout,Cin] bf16, bias [Cout] fp32 or None -> y [N,H,W,Cout] bf16
    (fp32 with ``out_f32``), H = 2 Hin with ``ups``.  ``pixelnorm`` raises ``ops.Unsupported`` above ``PIXELNORM_MAX_COUT`` couts."""
    cout, cin = w.shape[2], w.shape[3]
    H, W = (2 * Hin, 2 * Win) if ups else (Hin, Win)
    if tuple(x.shape) != (N, Hin, Win, cin) or tuple(w.shape[:2]) != (3, 3):
        raise ValueError('conv3_bf16: x %s against N, Hin, Win = %s and w %s' % (tuple(x.shape), (N, Hin, Win), tuple(w.shape)))
    y = torch.empty((N, H, W, cout), device=x.device, dtype=_F32 if out_f32 else _BF16)
    flags = (FLAG_UPSAMPLE if ups else 0) | (FLAG_PIXELNORM if pixelnorm else 0) | (FLAG_OUT_F32 if out_f32 else 0)
    _lib.call('pg_smp_conv3_bf16', _ptr(x, _BF16, 'x'), _ptr(w, _BF16, 'w'), _ptr(bias, _F32, 'bias'), _ptr(y, y.dtype, 'y'),
              N, Hin, Win, cin, cout, flags, scale, slope, eps, ops._stream())
    return y


def pixelnorm_bf16(x, eps=1e-8):
    """x [..., C] fp32 -> bf16, rne(x / sqrt(mean_c x^2 + eps)): the second launch of a layer too wide for the fused form."""
    C = x.shape[-1]
    y = torch.empty(x.shape, device=x.device, dtype=_BF16)
    _lib.call('pg_smp_pixelnorm_bf16', _ptr(x, _F32, 'x'), _ptr(y, _BF16, 'y'), x.numel() // C, C, eps, ops._stream())
    return y


def torgb_bf16(x, w, bias, N, C, H, W, scale, out_mul=1.0, prev=None, prev_w=None, prev_bias=None, prev_scale=1.0, prev_mul=0.0):
    """x [N,H,W,Cin] bf16, w [C,Cin] fp32 -> img [N,C,H,W] fp32 = out_mul (scale w.x + bias) + prev_mul (prev_scale prev_w.prev + prev_bias),
    ``prev`` [N,H/2,W/2,PCin] bf16 read at (h >> 1, w >> 1) (reference network.py:131-138)."""
    cin = w.shape[1]
    if tuple(x.shape) != (N, H, W, cin) or w.shape[0] != C:
        raise ValueError('torgb_bf16: x %s, w %s against N, C, H, W = %s' % (tuple(x.shape), tuple(w.shape), (N, C, H, W)))
    pcin = 0
    if prev is not None:
        pcin = prev_w.shape[1]
        if tuple(prev.shape) != (N, H // 2, W // 2, pcin) or prev_w.shape[0] != C:
            raise ValueError('torgb_bf16: prev %s, prev_w %s' % (tuple(prev.shape), tuple(prev_w.shape)))
    img = torch.empty((N, C, H, W), device=x.device, dtype=_F32)
    _lib.call('pg_smp_torgb_bf16', _ptr(x, _BF16, 'x'), _ptr(w, _F32, 'w'), _ptr(bias, _F32, 'bias'), scale, out_mul,
              _ptr(prev, _BF16, 'prev'), _ptr(prev_w, _F32, 'prev_w') if prev is not None else None,
              _ptr(prev_bias, _F32, 'prev_bias') if prev is not None else None, prev_scale, prev_mul, pcin,
              _ptr(img, _F32, 'img'), N, C, H, W, cin, ops._stream())
    return img


# ------------------------------------------------------------------------------------ the sampler
def _conv3_layers(net):
    """(name, layer) of every 3x3 layer of a generator, in evaluation order: all of its convs but block 0's c1."""
    return net.stage_convs(len(net.blocks))[1:]


class Sampler(object):
    """``Sampler(net)``: the bf16 evaluation of a ``Generator`` (``G`` or ``GeneratorEMA.network()``).  ``forward(z)`` / ``__call__``: fp32
    latents ``[N, latent]`` -> fp32 image ``[N, C, r, r]`` at ``net.depth`` / ``net.alpha`` as they are at the call.  An object of its own:
    it sets nothing on the network or its layers, and refers to the network weakly (``sampler_for`` keeps one per network).  Honours
    ``normalize_latents``, ``pixelnorm=False`` and ``leakyrelu=False``.  Raises ``ValueError`` at construction when a 3x3 layer's channel
    counts are not multiples of 8 (the MFMA fragment is 8 channels), naming the layer."""

    def __init__(self, net):
        if getattr(net, '_flat_param', None) is None or not hasattr(net, 'block0') or not hasattr(net, 'blocks'):
            raise ValueError('Sampler needs a Generator of this package (one flat parameter buffer); got %s' % type(net).__name__)
        for name, lay in _conv3_layers(net):
            if lay.ksize != 3 or lay.pad != 1:
                raise ValueError('Sampler: layer %s is %dx%d pad %d, not a 3x3 pad-1 conv' % (name, lay.ksize, lay.ksize, lay.pad))
            if lay.cin_store % 8 or lay.ch_out % 8:
                raise ValueError('Sampler: layer %s has %d -> %d channels; the bf16 kernels need multiples of 8'
                                 % (name, lay.cin_store, lay.ch_out))
        if not 1 <= int(net.num_channels) <= TORGB_MAX_C:
            raise ValueError('Sampler: %d image channels (1 .. %d)' % (net.num_channels, TORGB_MAX_C))
        self._net = weakref.ref(net)
        self._twin = None                # bf16 copy of the flat parameter buffer, same element offsets
        self._seen = None                # (address of the flat buffer, net._param_version) of the last cast
        self._offsets = None             # id(layer) -> element offset of its weight in the flat buffer

    def network(self):
        net = self._net()
        if net is None:
            raise RuntimeError('the network of this Sampler is gone')
        return net

    def _refresh(self, net):
        flat = net._flat_param
        if self._twin is None or self._twin.device != flat.device or self._twin.numel() != flat.numel() or self._seen[0] != flat.data_ptr():
            self._twin = torch.empty(flat.numel(), device=flat.device, dtype=_BF16)
            self._offsets = {}
            for name, lay in _conv3_layers(net):
                off = (lay.conv.weight.data_ptr() - flat.data_ptr()) // 4
                if off % 8:
                    raise ValueError('Sampler: the weight of %s sits at element %d of the flat buffer, not a multiple of 8' % (name, off))
                self._offsets[id(lay)] = off
            self._seen = None
        key = (flat.data_ptr(), net._param_version)
        if self._seen != key:
            cast_bf16(flat, self._twin)
            self._seen = key

    def _weight(self, lay):
        w = lay.conv.weight
        off = self._offsets[id(lay)]
        return self._twin[off:off + w.numel()].view(w.shape)

    def _layer(self, x, lay, N, H, ups=False):
        """One 3x3 layer of the contract at output size H: the fused launch, or conv to fp32 + PixelNorm where that answers PG_E_UNSUP."""
        w, b = self._weight(lay), lay.conv.bias.data
        Hin = H // 2 if ups else H
        if not lay.pixelnorm:
            return conv3_bf16(x, w, b, N, Hin, Hin, lay.c, lay.slope, lay.eps, ups=ups)
        try:
            return conv3_bf16(x, w, b, N, Hin, Hin, lay.c, lay.slope, lay.eps, ups=ups, pixelnorm=True)
        except ops.Unsupported:
            y = conv3_bf16(x, w, b, N, Hin, Hin, lay.c, lay.slope, lay.eps, ups=ups, out_f32=True)
            return pixelnorm_bf16(y, lay.eps)

    def forward(self, z, return_activations=False):
        """``return_activations``: also the list of the bf16 layer outputs in evaluation order (block 0's c1 first): (img, acts)."""
        net = self.network()
        engine.wait_pending(net)
        ops.require_gpu()
        net._sync_version()               # also notice torch-side updates (torch.optim.*, load_state_dict) before the twin is judged
        z = engine._check_dev(z, 'latents')
        N, L = z.shape
        if L != net.latent_size or L % 4:
            raise ValueError('latent size %d (expected %d, multiple of 4)' % (L, net.latent_size))
        depth, alpha = int(net.depth), float(net.alpha)
        C = int(net.num_channels)
        self._refresh(net)
        zn = ops.pixelnorm_fwd(z, net.eps)[0] if net.normalize_latents else z
        b0 = net.block0
        c1 = b0.c1                        # the 4x4 conv on the 1x1 latent: fp32 path, rounded once
        if c1.pixelnorm:
            y1 = ops.conv2d_pixelnorm(zn.view(N, 1, 1, L), c1.conv.weight.data, c1.conv.bias.data, N, 1, 1, c1.ksize, c1.pad, c1.c,
                                      c1.slope, c1.eps)[0]
        else:
            y1 = ops.conv2d(zn.view(N, 1, 1, L), c1.conv.weight.data, c1.conv.bias.data, N, 1, 1, c1.ksize, c1.pad, c1.c, c1.slope)
        h = cast_bf16(y1)
        acts = [h]
        h = self._layer(h, b0.c2, N, 4)
        acts.append(h)
        H, hprev = 4, None
        for i in range(depth):
            blk = net.blocks[i]
            H *= 2
            a1 = self._layer(h, blk.c1, N, H, ups=True)
            a2 = self._layer(a1, blk.c2, N, H)
            acts += [a1, a2]
            hprev, h = h, a2
        t, pt = net.rgb_heads(depth, alpha)
        if pt is not None:
            img = torgb_bf16(h, t.conv.weight.data, t.conv.bias.data, N, C, H, H, t.c, out_mul=alpha, prev=hprev,
                             prev_w=pt.conv.weight.data, prev_bias=pt.conv.bias.data, prev_scale=pt.c, prev_mul=1.0 - alpha)
        else:
            img = torgb_bf16(h, t.conv.weight.data, t.conv.bias.data, N, C, H, H, t.c)
        return (img, acts) if return_activations else img

    __call__ = forward


_SAMPLERS = weakref.WeakKeyDictionary()        # network -> its Sampler (which refers back weakly: an entry dies with its network)


def sampler_for(net):
    """The ``Sampler`` of a network, made at the first request and kept as long as the network lives."""
    s = _SAMPLERS.get(net)
    if s is None:
        s = _SAMPLERS[net] = Sampler(net)
    return s


def check_precision(precision, who='precision'):
    if precision not in PRECISIONS:
        raise ValueError("%s must be 'fp32' or 'bf16', got %r" % (who, precision))
    return precision


def generator_for(net, precision='fp32'):
    """What a consumer calls ``.forward(z)`` on: the network itself ('fp32') or its sampler ('bf16')."""
    return net if check_precision(precision) == 'fp32' else sampler_for(net)
