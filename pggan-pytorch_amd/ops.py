"""Tensor-level wrappers of the C-ABI kernels (include/pggan_hip.h).

PyTorch is used only as the device allocator and stream provider: every function takes fp32
CUDA(HIP) tensors, allocates its output with ``torch.empty`` and launches a hand-written HIP
kernel on the current stream.  No ATen arithmetic, no CPU fallback.
Feature tensors are NHWC ``[N,H,W,C]``; image tensors are NCHW ``[N,C,H,W]``."""
import os as _os

import ctypes

import torch

from . import _lib

_C = _lib.CONSTANTS          # every #define PG_* that include/pggan_hip.h carries


def _stream():
    """Raw HIP stream handle of torch's current stream.  torch.cuda.current_stream() costs ~17 us per call (device
    index resolution through is_available() / os.environ) and this is called once per kernel launch (~400 per step)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


# Scratch of the launches that slice K across workgroups (include/pggan_hip.h: pg_set_workspace), one per (device, stream),
# zero-filled, registered with the library the first time a conv is launched on that stream and kept for good.  Streams that are
# being captured into a hipGraph (a new stream per capture) all share ONE more buffer per device, allocated eagerly the first time
# any eager stream gets its own: the engine replays its graphs one after the other, and a buffer allocated inside a capture would
# belong to that graph's memory pool.
WORKSPACE_BYTES = int(_os.environ.get('PGGAN_WORKSPACE_MB', '32')) << 20
_workspaces = {}
_capture_workspace = {}
_no_workspace_streams = set()     # raw handles of streams that must never carry a scratch launch while a graph is captured (engine's side stream)


def workspace_bytes(kind, N, H, W, cin, cout):
    """Scratch the launch of that shape uses when at least as much is registered (pg_workspace_bytes; 0: it never slices).
    kind 0: conv2d_wino, kind 1: the 4x4 valid conv on a 4x4 map."""
    n = ctypes.c_size_t(0)
    _lib.call('pg_workspace_bytes', kind, N, H, W, cin, cout, ctypes.addressof(n))
    return int(n.value)


def _stream_with_workspace():
    """Raw handle of the current stream, with a scratch registered for it (pg_set_workspace).  The scratch carries self-resetting
    tickets, so it belongs to ONE stream; the streams of hipGraph captures share one more per device, which is correct because a
    captured graph of this package has a single branch that launches scratch kernels (the main stream: weight gradients, Adam and
    derived weights on the forked side stream never slice) and graphs replay one after the other -- the first condition is
    enforced here, the second by the engine replaying on one stream."""
    dev = torch._C._cuda_getDevice()
    s = torch._C._cuda_getCurrentRawStream(dev)
    if (dev, s) not in _workspaces:
        ws = None
        capturing = torch.cuda.is_current_stream_capturing()
        if WORKSPACE_BYTES > 0:
            if capturing:
                if s in _no_workspace_streams:
                    raise RuntimeError('a scratch (K-sliced) launch on the forked side stream of a hipGraph capture: the capture '
                                       'streams of a device share one scratch, so only one branch of a graph may slice')
                ws = _capture_workspace.get(dev)             # (None before the first eager launch: this launch runs unsplit)
            else:
                ws = torch.zeros(WORKSPACE_BYTES, dtype=torch.uint8, device='cuda:%d' % dev)
                if dev not in _capture_workspace:
                    _capture_workspace[dev] = torch.zeros(WORKSPACE_BYTES, dtype=torch.uint8, device='cuda:%d' % dev)
        if ws is not None:
            _lib.call('pg_set_workspace', s, ws.data_ptr(), ws.numel())
        if ws is None and capturing:
            return s                                         # not cached: a later capture on a stream with this handle gets the scratch
        _workspaces[(dev, s)] = ws
    return s


def release_capture_workspaces():
    """Forget (and unregister) the scratch entries of capture streams: called when the captured graphs are dropped
    (graphs.clear), whose streams are gone -- a later stream may reuse the raw handle."""
    shared = set(id(t) for t in _capture_workspace.values())
    for (dev, s), ws in list(_workspaces.items()):
        if ws is not None and id(ws) in shared:
            with torch.cuda.device(dev):
                _lib.call('pg_set_workspace', s, None, 0)
            del _workspaces[(dev, s)]


_F32, _U8 = torch.float32, torch.uint8


def _p(t):
    """Device pointer of a checked tensor (None -> NULL)."""
    if t is None:
        return None
    dt = t.dtype
    if not t.is_cuda or (dt is not _F32 and dt is not _U8) or not t.is_contiguous():
        raise ValueError('expected a contiguous fp32 (or sign-byte uint8) device tensor, got %s %s contiguous=%s on %s'
                         % (tuple(t.shape), t.dtype, t.is_contiguous(), t.device))
    return t.data_ptr()


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError('pggan-pytorch_amd needs an MI355X (gfx950) device: the hot path has no CPU fallback')
    _lib.load()


# ------------------------------------------------------------------------------------ output allocation
# The D step evaluates the real, fake and mixed thirds of its [real | fake | mixed] batch as THREE passes of engine.d_forward (on two
# streams) that must leave their outputs in ONE set of batched tensors: inside an ``Arena`` context the forward ops below take their
# outputs from the arena instead of the allocator.  The first pass (part 0, leading extent n) creates every buffer with leading extent 3n
# and gets rows [0, n); the passes of the fake and the mixed third (parts 2 and 3) walk the same buffers in the same order and get rows
# [n, 2n) and [2n, 3n).  Buffers are kept for the next iteration (the launch plans bake their addresses).  Outside a context: torch.empty.
_ARENA = None


def _empty(shape, device=None, dtype=torch.float32):
    a = _ARENA
    if a is None:
        return torch.empty(shape, device=device, dtype=dtype)
    return a.take(tuple(shape), device, dtype)


class Arena(object):
    def __init__(self):
        self.bufs = []
        self.i = 0
        self.part = None

    def take(self, shape, device, dtype):
        lead, rest = shape[0], shape[1:]
        if self.part == 0:
            if self.i == len(self.bufs):
                self.bufs.append(torch.empty((3 * lead,) + rest, device=device, dtype=dtype))
            big = self.bufs[self.i]
            unit = lead
        else:
            if self.i >= len(self.bufs) or (self.part == 1 and lead % 2):
                raise RuntimeError('split D forward: the second pass asks for an output the first pass did not create')
            big = self.bufs[self.i]
            unit = lead // 2 if self.part == 1 else lead
        if tuple(big.shape) != (3 * unit,) + rest or big.dtype != dtype:
            raise RuntimeError('split D forward: output %d differs between the passes (%s %s vs %s x3)' % (self.i, tuple(big.shape), big.dtype, shape))
        self.i += 1
        # part 0: first third | 1: second and third thirds in one pass | 2 / 3: the second / the third third alone
        return big[:unit] if self.part == 0 else big[unit:] if self.part == 1 else big[unit:2 * unit] if self.part == 2 else big[2 * unit:]

    def pass_(self, part):
        return _ArenaPass(self, part)


class _ArenaPass(object):
    def __init__(self, arena, part):
        self.arena, self.part = arena, part

    def __enter__(self):
        global _ARENA
        if _ARENA is not None:
            raise RuntimeError('nested output arenas')
        self.arena.part, self.arena.i = self.part, 0
        _ARENA = self.arena
        return self.arena

    def __exit__(self, *exc):
        global _ARENA
        _ARENA = None
        if exc[0] is None and self.arena.i != len(self.arena.bufs):
            raise RuntimeError('split D forward: the passes created a different number of outputs (%d of %d)' % (self.arena.i, len(self.arena.bufs)))
        return False


# ------------------------------------------------------------------------------------ conv
def _is_bytes(t):
    return t is not None and t.dtype == torch.uint8


FLAG_UPSAMPLE, FLAG_MASK_BYTES = _C['PG_FLAG_UPSAMPLE'], _C['PG_FLAG_MASK_BYTES']
FLAG_Y_BYTES, FLAG_SIGNS_OUT = _C['PG_FLAG_Y_BYTES'], _C['PG_FLAG_SIGNS_OUT']
Unsupported = _lib.Unsupported


def conv2d(x, w, bias, N, Hin, Win, ks, pad, scale, slope=1.0, mask=None, mask_slope=0.2, ups=False,
           out=None, signs_out=False):
    """x: [N,Hin(/2),Win(/2),Cin]; w packed [ks,ks,Cout,Cin] -> y [N,Hout,Wout,Cout].  A uint8 ``mask`` holds sign bytes;
    ``signs_out`` (forward mode) additionally returns the sign bytes of y: (y, bytes).  Both may raise ops.Unsupported."""
    cout, cin = w.shape[2], w.shape[3]
    ho, wo = Hin + 2 * pad - ks + 1, Win + 2 * pad - ks + 1
    y = out if out is not None else _empty((N, ho, wo, cout), device=x.device, dtype=torch.float32)
    flags = (FLAG_UPSAMPLE if ups else 0) | (FLAG_MASK_BYTES if _is_bytes(mask) else 0)
    sb = None
    if signs_out:
        sb = _empty((N, ho, wo, cout // 4), device=x.device, dtype=torch.uint8)
        mask, flags = sb, flags | FLAG_SIGNS_OUT
    _lib.call('pg_conv2d_nhwc', _p(x), _p(w), _p(bias), _p(mask), _p(y), N, Hin, Win, cin, cout, ks, pad,
              flags, scale, slope, mask_slope, _stream_with_workspace() if ks == 4 else _stream())
    return (y, sb) if signs_out else y


def wino_unpack(u):
    """Device layout of the Winograd-domain weights (8-channel packs, [Cin/8][16][Cout][8], csrc/conv_wino.hip::wino_u_index)
    -> plain [16, Cout, Cin] (tests / diagnostics)."""
    _, cout, cin = u.shape
    return u.reshape(cin // 8, 16, cout, 8).permute(1, 2, 0, 3).reshape(16, cout, cin)


def wino_transform_weights(w, u=None):
    """w packed [3,3,Cout,Cin] -> Winograd-domain weights u, nominal shape [16,Cout,Cin], stored in 8-channel packs (``wino_unpack``)."""
    ks, _, cout, cin = w.shape
    assert ks == 3
    if u is None:
        u = torch.empty((16, cout, cin), device=w.device, dtype=torch.float32)
    _lib.call('pg_wino_transform_weights', _p(w), _p(u), cout, cin, _stream())
    return u


def wino_transform_weights_batched(flat_w, flat_u, layers, transposed=False):
    """layers: [(w element offset in flat_w, u element offset in flat_u, cout, cin), ...]; one launch.  ``transposed``: every
    layer is the backward-data form of a forward layer, computed straight from that layer's parameter (cout / cin are those of
    the backward-data conv, i.e. the forward layer's cin / cout)."""
    n = len(layers)
    if n == 0:
        return
    woff = (ctypes.c_int64 * n)(*[l[0] for l in layers])
    uoff = (ctypes.c_int64 * n)(*[l[1] for l in layers])
    co = (ctypes.c_int * n)(*[l[2] for l in layers])
    ci = (ctypes.c_int * n)(*[l[3] for l in layers])
    if isinstance(transposed, (list, tuple)):          # per-layer flags: forward and backward-data forms of a network in one launch
        tr = (ctypes.c_int * n)(*[1 if t else 0 for t in transposed]) if any(transposed) else None
    else:
        tr = (ctypes.c_int * n)(*([1] * n)) if transposed else None
    _lib.call('pg_wino_transform_weights_batched', _p(flat_w), _p(flat_u), n, ctypes.cast(woff, ctypes.c_void_p),
              ctypes.cast(uoff, ctypes.c_void_p), ctypes.cast(co, ctypes.c_void_p), ctypes.cast(ci, ctypes.c_void_p),
              ctypes.cast(tr, ctypes.c_void_p) if tr is not None else None, _stream())


def signbytes_to_mask(b):
    """uint8 sign bytes [..., C/4] -> fp32 +1/-1 mask [..., C] (fallback when an entry point does not take sign bytes)."""
    m = torch.empty(tuple(b.shape[:-1]) + (4 * b.shape[-1],), device=b.device, dtype=torch.float32)
    _lib.call('pg_signbytes_to_mask', _p(b), _p(m), b.numel(), _stream())
    return m


def conv2d_wino(x, u, bias, N, H, W, scale, slope=1.0, mask=None, mask_slope=0.2, ups=False, out=None,
                pool=False, other=None, a=1.0, b=0.0, pool_only=False, unpool=False, upmask=None, up_mul=1.0, y_bytes=False,
                signs_out=False):
    """3x3 pad-1 conv on Winograd-domain weights (+ the fused pool / unpool epilogues).  Returns y, (y, ypool) or yup.
    uint8 ``mask`` / ``upmask`` are sign bytes; ``y_bytes`` (with ``pool``) returns the sign bytes of y instead of y."""
    cout, cin = u.shape[1], u.shape[2]
    flags = (FLAG_UPSAMPLE if ups else 0) | (FLAG_MASK_BYTES if _is_bytes(mask) or _is_bytes(upmask) else 0) | (FLAG_Y_BYTES if y_bytes else 0)
    if y_bytes:
        y = _empty((N, H, W, cout // 4), device=x.device, dtype=torch.uint8)
    else:
        y = out if out is not None else _empty((N, H, W, cout), device=x.device, dtype=torch.float32)
    yp = _empty((N, H // 2, W // 2, cout), device=x.device, dtype=torch.float32) if pool else None
    yu = _empty((N, 2 * H, 2 * W, cout), device=x.device, dtype=torch.float32) if unpool else None
    sb = None
    if signs_out:                                  # plain forward launch: (y, sign bytes of y)
        sb = _empty((N, H, W, cout // 4), device=x.device, dtype=torch.uint8)
        mask, flags = sb, flags | FLAG_SIGNS_OUT
    _lib.call('pg_conv2d_wino_nhwc', _p(x), _p(u), _p(bias), _p(mask), _p(y), _p(yp), _p(other), a, b, 1 if pool_only else 0,
              _p(yu), _p(upmask), up_mul, N, H, W, cin, cout, flags, scale, slope, mask_slope, _stream_with_workspace())
    if signs_out:
        return y, sb
    if pool:
        return y, yp
    if unpool:
        return yu
    return y


def conv2d_wino_pixelnorm(x, u, bias, N, H, W, scale, slope, eps=1e-8, ups=False):
    """conv2d_pixelnorm on Winograd-domain weights (3x3 pad 1, at most 32 couts: ops.Unsupported otherwise).  Returns (y, r)."""
    cout, cin = u.shape[1], u.shape[2]
    y = torch.empty((N, H, W, cout), device=x.device, dtype=torch.float32)
    r = torch.empty((N * H * W,), device=x.device, dtype=torch.float32)
    _lib.call('pg_conv2d_wino_pixelnorm_nhwc', _p(x), _p(u), _p(bias), _p(y), _p(r), N, H, W, cin, cout, 1 if ups else 0,
              scale, slope, eps, _stream())
    return y, r


def conv2d_wino_pnbwd(x, u, ysaved, r, N, H, W, scale, slope, pool=False, other=None, a=1.0, b=0.0):
    """Backward-data conv on Winograd-domain weights (+ 2x2 pool blend a * pool + b * other) + the adjoint of the previous layer's
    (LeakyReLU -> PixelNorm), one launch; at most 32 couts (ops.Unsupported otherwise)."""
    cout, cin = u.shape[1], u.shape[2]
    y = torch.empty((N, H // 2, W // 2, cout) if pool else (N, H, W, cout), device=x.device, dtype=torch.float32)
    _lib.call('pg_conv2d_wino_pnbwd_nhwc', _p(x), _p(u), _p(ysaved), _p(r), _p(y), 1 if pool else 0, _p(other), a, b,
              N, H, W, cin, cout, scale, slope, _stream())
    return y


def conv2d_pool(x, w, bias, N, Hin, Win, ks, pad, scale, slope=1.0, mask=None, mask_slope=0.2, other=None, a=1.0, b=0.0,
                pool_only=False, y_bytes=False):
    """conv2d with the following 2x2 average pool (+ fade-in blend a*pool + b*other) fused into the epilogue.
    Returns (y, ypool); with ``pool_only`` the full-resolution y may be left unwritten (do not read it).  A uint8
    ``mask`` holds sign bytes; ``y_bytes`` returns the sign bytes of y instead of y (raises ops.Unsupported when the
    launch cannot fuse -- redo with fp32)."""
    cout, cin = w.shape[2], w.shape[3]
    ho, wo = Hin + 2 * pad - ks + 1, Win + 2 * pad - ks + 1
    flags = (FLAG_MASK_BYTES if _is_bytes(mask) else 0) | (FLAG_Y_BYTES if y_bytes else 0)
    if y_bytes:
        y = _empty((N, ho, wo, cout // 4), device=x.device, dtype=torch.uint8)
    else:
        y = _empty((N, ho, wo, cout), device=x.device, dtype=torch.float32)
    yp = _empty((N, ho // 2, wo // 2, cout), device=x.device, dtype=torch.float32)
    _lib.call('pg_conv2d_pool_nhwc', _p(x), _p(w), _p(bias), _p(mask), _p(y), _p(yp), _p(other), a, b, 1 if pool_only else 0,
              N, Hin, Win, cin, cout, ks, pad, flags, scale, slope, mask_slope, _stream())
    return y, yp


def conv2d_pixelnorm(x, w, bias, N, Hin, Win, ks, pad, scale, slope, eps=1e-8, ups=False):
    """conv -> bias -> LeakyReLU -> PixelNorm in one launch where the tile shape allows it.  Returns (y, r)."""
    cout, cin = w.shape[2], w.shape[3]
    ho, wo = Hin + 2 * pad - ks + 1, Win + 2 * pad - ks + 1
    y = torch.empty((N, ho, wo, cout), device=x.device, dtype=torch.float32)
    r = torch.empty((N * ho * wo,), device=x.device, dtype=torch.float32)
    _lib.call('pg_conv2d_pixelnorm_nhwc', _p(x), _p(w), _p(bias), _p(y), _p(r), N, Hin, Win, cin, cout, ks, pad,
              1 if ups else 0, scale, slope, eps, _stream())
    return y, r


def conv2d_pixelnorm_torgb(x, w, bias, t_w, t_b, N, C, H, W, scale, slope, t_scale, eps=1e-8, out=None):
    """conv2d_pixelnorm (3x3 pad 1) with the block's toRGB layer in the same epilogue.  t_w [C,Cout(,1,1)].  Returns (y, r, img
    [N,C,H,W]); raises ops.Unsupported outside the 8 -> 8 layer of the 1024^2 stage."""
    cout, cin = w.shape[2], w.shape[3]
    y = torch.empty((N, H, W, cout), device=x.device, dtype=torch.float32)
    r = torch.empty((N * H * W,), device=x.device, dtype=torch.float32)
    if out is None:
        out = torch.empty((N, C, H, W), device=x.device, dtype=torch.float32)
    _lib.call('pg_conv2d_pixelnorm_torgb_nhwc', _p(x), _p(w), _p(bias), _p(y), _p(r), _p(t_w), _p(t_b), t_scale, _p(out),
              N, C, H, W, cin, cout, scale, slope, eps, _stream())
    return y, r, out


def conv2d_pnbwd(x, w, ysaved, r, N, Hin, Win, ks, pad, scale, slope):
    """Backward-data conv + adjoint of the previous layer's (LeakyReLU -> PixelNorm) in one launch where possible."""
    cout, cin = w.shape[2], w.shape[3]
    ho, wo = Hin + 2 * pad - ks + 1, Win + 2 * pad - ks + 1
    y = torch.empty((N, ho, wo, cout), device=x.device, dtype=torch.float32)
    _lib.call('pg_conv2d_pnbwd_nhwc', _p(x), _p(w), _p(ysaved), _p(r), _p(y), N, Hin, Win, cin, cout, ks, pad, scale, slope, _stream())
    return y


def conv2d_unpool(x, w, N, Hin, Win, ks, pad, scale, upmask=None, mul=1.0, mask_slope=0.2):
    """Backward-data conv followed by the adjoint of the 2x2 average pool (x0.25*mul, nearest x2) and the
    LeakyReLU' mask of the finer activation, fused.  Returns the fine-resolution gradient [N,2Ho,2Wo,Cout]."""
    cout, cin = w.shape[2], w.shape[3]
    ho, wo = Hin + 2 * pad - ks + 1, Win + 2 * pad - ks + 1
    y = torch.empty((N, ho, wo, cout), device=x.device, dtype=torch.float32)          # scratch (unfused fallback)
    yup = torch.empty((N, 2 * ho, 2 * wo, cout), device=x.device, dtype=torch.float32)
    _lib.call('pg_conv2d_unpool_nhwc', _p(x), _p(w), _p(upmask), _p(y), _p(yup), N, Hin, Win, cin, cout, ks, pad,
              FLAG_MASK_BYTES if _is_bytes(upmask) else 0, scale, mul, mask_slope, _stream())
    return yup


def conv2d_unpooled(g, w, gbytes, gmul, gslope, N, Hin, Win, scale, mask=None, mask_slope=0.2):
    """Backward-data 3x3 conv whose input is the pool adjoint of ``g`` [N,Hin/2,Win/2,Cin] (x gmul, x LeakyReLU' from the sign
    bytes ``gbytes`` [N,Hin,Win,Cin/4]) evaluated in the gather.  w packed [3,3,Cout,Cin]; raises ops.Unsupported."""
    cout, cin = w.shape[2], w.shape[3]
    y = torch.empty((N, Hin, Win, cout), device=g.device, dtype=torch.float32)
    _lib.call('pg_conv2d_unpooled_nhwc', _p(g), _p(w), _p(gbytes), gmul, gslope, _p(mask), _p(y), N, Hin, Win, cin, cout,
              FLAG_MASK_BYTES if _is_bytes(mask) else 0, scale, mask_slope, _stream())
    return y


def conv2d_fromrgb(img, rgb_w, rgb_b, rgb_scale, rgb_slope, w, bias, N, C, H, W, scale, slope, signs_out=True):
    """c1(fromRGB(img)) of a DBlock in one launch, fromRGB evaluated in the conv's gather (its fp32 output is never written).
    img [N,C,H,W], rgb_w [Cmid,C,1,1] / [Cmid,C], w packed [3,3,Cout,Cmid].  Returns (y, sign bytes of y, sign bytes of fromRGB's
    output); raises ops.Unsupported outside the 8 -> 8 layer of the 1024^2 stage."""
    cout, cmid = w.shape[2], w.shape[3]
    y = _empty((N, H, W, cout), device=img.device, dtype=torch.float32)
    yb = _empty((N, H, W, cout // 4), device=img.device, dtype=torch.uint8) if signs_out else None
    xb = _empty((N, H, W, cmid // 4), device=img.device, dtype=torch.uint8)
    _lib.call('pg_conv2d_fromrgb_nhwc', _p(img), _p(rgb_w), _p(rgb_b), rgb_scale, rgb_slope, _p(xb), _p(w), _p(bias), _p(y), _p(yb),
              N, C, H, W, cmid, cout, scale, slope, _stream())
    return y, yb, xb


def conv2d_masked_fromrgb_bwd(gz, wt, mask_bytes, mask_slope, rgb_w, rgb_scale, N, C, H, W, scale, keep_gf=True, gimg=None, want_gimg=True,
                              img=None, rgb_dw=None, rgb_db=None):
    """Backward-data conv of a DBlock's c1 (x LeakyReLU' from the sign bytes of fromRGB's output) with fromRGB's backward-data
    (``want_gimg``) and / or fromRGB's weight + bias gradient (``img``, ``rgb_dw``, ``rgb_db``: accumulated into) in the epilogue.
    wt: flipped / transposed weights [3,3,Cin',Cout'].  Returns (gf [N,H,W,8] or None, gimg [N,C,H,W] or None); raises ops.Unsupported
    outside the 8 -> 8 layer of the 1024^2 stage."""
    cout, cin = wt.shape[2], wt.shape[3]
    gf = _empty((N, H, W, cout), device=gz.device, dtype=torch.float32) if keep_gf else None
    if gimg is None and want_gimg:
        gimg = torch.empty((N, C, H, W), device=gz.device, dtype=torch.float32)
    _lib.call('pg_conv2d_masked_fromrgb_bwd_nhwc', _p(gz), _p(wt), _p(mask_bytes), mask_slope, _p(gf), _p(rgb_w), rgb_scale, _p(gimg),
              _p(img), _p(rgb_dw), _p(rgb_db), N, C, H, W, cin, cout, scale, _stream())
    return gf, gimg



def conv2d_wgrad_unpooled(x, g, gbytes, gmul, gslope, dw, db, N, Hin, Win, scale):
    """Weight gradient with gz = pool adjoint of ``g`` evaluated in the gather (see conv2d_unpooled)."""
    cout, cin = dw.shape[2], dw.shape[3]
    _lib.call('pg_conv2d_wgrad_unpooled_nhwc', _p(x), _p(g), _p(gbytes), gmul, gslope, _p(dw), _p(db), N, Hin, Win, cin, cout,
              scale, _stream())


def conv2d_wgrad(x, gz, dw, db, N, Hin, Win, ks, pad, scale, ups=False):
    """Accumulates into dw [ks,ks,Cout,Cin] (and db [Cout] if given)."""
    cout, cin = dw.shape[2], dw.shape[3]
    _lib.call('pg_conv2d_wgrad_nhwc', _p(x), _p(gz), _p(dw), _p(db), N, Hin, Win, cin, cout, ks, pad,
              1 if ups else 0, scale, _stream())


def conv2d_wgrad_wino(x, gz, dw, db, N, H, W, scale, ups=False, second=None):
    """Winograd form of conv2d_wgrad for 3x3 pad-1 layers: accumulates into dw [3,3,Cout,Cin] (and db).
    ``second`` = (x2, gz2, N2, bias2): another batch of the same layer summed in the same launch (one commit of dW);
    its gz joins db when ``bias2``."""
    cout, cin = dw.shape[2], dw.shape[3]
    if second is None:
        _lib.call('pg_conv2d_wgrad_wino_nhwc', _p(x), _p(gz), _p(dw), _p(db), N, H, W, cin, cout, 1 if ups else 0, scale, _stream())
        return
    x2, gz2, n2, bias2 = second
    _lib.call('pg_conv2d_wgrad_wino2_nhwc', _p(x), _p(gz), N, _p(x2), _p(gz2), n2, _p(dw), _p(db),
              (1 if db is not None else 0) | (2 if (bias2 and db is not None) else 0), H, W, cin, cout, 1 if ups else 0, scale, _stream())


def pack_dgrad_weights(w, wt):
    ks, _, cout, cin = w.shape
    _lib.call('pg_pack_dgrad_weights', _p(w), _p(wt), ks, cout, cin, _stream())
    return wt


def pack_dgrad_weights_batched(flat_w, flat_wt, layers):
    """layers: [(element offset, ks, cout, cin), ...] inside the flat weight buffer / its mirror; one launch."""
    n = len(layers)
    off = (ctypes.c_int64 * n)(*[l[0] for l in layers])
    ks = (ctypes.c_int * n)(*[l[1] for l in layers])
    co = (ctypes.c_int * n)(*[l[2] for l in layers])
    ci = (ctypes.c_int * n)(*[l[3] for l in layers])
    _lib.call('pg_pack_dgrad_weights_batched', _p(flat_w), _p(flat_wt), n, ctypes.cast(off, ctypes.c_void_p),
              ctypes.cast(ks, ctypes.c_void_p), ctypes.cast(co, ctypes.c_void_p), ctypes.cast(ci, ctypes.c_void_p), _stream())


# --------------------------------------------------------------------------------- from/toRGB
def fromrgb_fwd(img, w, bias, N, C, H, W, scale, slope, pool=False, mask=None, mask_slope=0.2, signs_out=False):
    cout = w.shape[0]
    y = _empty((N, H, W, cout), device=img.device, dtype=torch.float32)
    flags = (1 if pool else 0) | (FLAG_MASK_BYTES if _is_bytes(mask) else 0)
    sb = None
    if signs_out:
        sb = _empty((N, H, W, cout // 4), device=img.device, dtype=torch.uint8)
        mask, flags = sb, flags | FLAG_SIGNS_OUT
    _lib.call('pg_fromrgb_fwd', _p(img), _p(w), _p(bias), _p(mask), _p(y), N, C, H, W, cout, flags,
              scale, slope, mask_slope, _stream())
    return (y, sb) if signs_out else y


def fromrgb_bwd_data(gz, w, gimg, N, C, H, W, scale, pool=False, accumulate=False):
    cout = w.shape[0]
    _lib.call('pg_fromrgb_bwd_data', _p(gz), _p(w), _p(gimg), N, C, H, W, cout, 1 if pool else 0,
              1 if accumulate else 0, scale, _stream())


def fromrgb_wgrad(gz, img, dw, db, N, C, H, W, scale, pool=False):
    cout = dw.shape[0]
    _lib.call('pg_fromrgb_wgrad', _p(gz), _p(img), _p(dw), _p(db), N, C, H, W, cout, 1 if pool else 0, scale, _stream())


def torgb_fwd(x, w, bias, N, C, H, W, scale, out_mul=1.0, prev=None, prev_mul=0.0, out=None):
    cin = w.shape[1]
    if out is None:
        out = torch.empty((N, C, H, W), device=x.device, dtype=torch.float32)
    _lib.call('pg_torgb_fwd', _p(x), _p(w), _p(bias), _p(prev), _p(out), N, C, H, W, cin, scale, out_mul, prev_mul, _stream())
    return out


def torgb_bwd_data(g, w, N, C, H, W, mul_scale, down=False):
    cin = w.shape[1]
    gx = torch.empty((N, H, W, cin), device=g.device, dtype=torch.float32)
    _lib.call('pg_torgb_bwd_data', _p(g), _p(w), _p(gx), N, C, H, W, cin, 1 if down else 0, mul_scale, _stream())
    return gx


def torgb_bwd_data_pnbwd(g, w, ysaved, r, N, C, H, W, mul_scale, slope):
    """torgb_bwd_data + the adjoint of the block's (LeakyReLU -> PixelNorm), one launch where the kernel exists, two otherwise."""
    cin = w.shape[1]
    gx = torch.empty((N, H, W, cin), device=g.device, dtype=torch.float32)
    try:
        _lib.call('pg_torgb_bwd_data_pnbwd', _p(g), _p(w), _p(ysaved), _p(r), _p(gx), N, C, H, W, cin, mul_scale, slope, _stream())
        return gx
    except Unsupported:
        return pixelnorm_lrelu_bwd(torgb_bwd_data(g, w, N, C, H, W, mul_scale), ysaved, r, slope, inplace=True)


def torgb_wgrad(g, x, dw, db, N, C, H, W, mul_scale, mul, down=False):
    cin = dw.shape[1]
    _lib.call('pg_torgb_wgrad', _p(g), _p(x), _p(dw), _p(db), N, C, H, W, cin, 1 if down else 0, mul_scale, mul, _stream())


# --------------------------------------------------------------------------- pool / upsample
def avgpool2_fwd(x, other=None, a=1.0, b=0.0):
    N, H2, W2, C = x.shape
    y = torch.empty((N, H2 // 2, W2 // 2, C), device=x.device, dtype=torch.float32)
    _lib.call('pg_avgpool2_fwd', _p(x), _p(other), _p(y), N, H2 // 2, W2 // 2, C, a, b, _stream())
    return y


def avgpool2_bwd(gy, mask=None, mul=1.0, mask_slope=0.2):
    N, H, W, C = gy.shape
    gx = torch.empty((N, 2 * H, 2 * W, C), device=gy.device, dtype=torch.float32)
    _lib.call('pg_avgpool2_bwd', _p(gy), _p(mask), _p(gx), N, H, W, C, mul, mask_slope, _stream())
    return gx


def upsample2_bwd(g):
    N, H2, W2, C = g.shape
    gx = torch.empty((N, H2 // 2, W2 // 2, C), device=g.device, dtype=torch.float32)
    _lib.call('pg_upsample2_bwd', _p(g), _p(gx), N, H2 // 2, W2 // 2, C, _stream())
    return gx


def axpby_mask(x, other=None, mask=None, a=1.0, b=0.0, mask_slope=0.2, out=None):
    y = out if out is not None else torch.empty_like(x)
    _lib.call('pg_axpby_mask', _p(x), _p(other), _p(mask), _p(y), x.numel(), a, b, mask_slope, _stream())
    return y


# ---------------------------------------------------------------------------------- pixelnorm
def pixelnorm_fwd(x, eps=1e-8, inplace=False):
    C = x.shape[-1]
    P = x.numel() // C
    y = x if inplace else torch.empty_like(x)
    r = torch.empty((P,), device=x.device, dtype=torch.float32)
    _lib.call('pg_pixelnorm_fwd', _p(x), _p(y), _p(r), P, C, eps, _stream())
    return y, r


def pixelnorm_lrelu_bwd(gy, y, r, slope, inplace=False, inj=None, out=None):
    C = y.shape[-1]
    P = y.numel() // C
    gz = out if out is not None else (gy if inplace else torch.empty_like(gy))
    if inj is None:
        _lib.call('pg_pixelnorm_lrelu_bwd', _p(gy), _p(y), _p(r), _p(gz), P, C, slope, _stream())
    else:
        _lib.call('pg_pixelnorm_lrelu_bwd_inj', _p(gy), _p(y), _p(r), _p(inj), _p(gz), P, C, slope, _stream())
    return gz


def pixelnorm_tangent(t, y, r, a):
    """(ty, inj) of pg_pixelnorm_tangent: tangent through PixelNorm and its Hessian-vector injection."""
    C = y.shape[-1]
    P = y.numel() // C
    ty, inj = torch.empty_like(t), torch.empty_like(t)
    _lib.call('pg_pixelnorm_tangent', _p(t), _p(y), _p(r), _p(a), _p(ty), _p(inj), P, C, _stream())
    return ty, inj


# -------------------------------------------------------------------------------------- mbstd
MBSTD_STATS_STRIDE = _C['PG_MBSTD_STATS_STRIDE']        # [mu, sigma, reduction workspace]


def mbstd_fwd(x, groups, cp):
    NB, H, W, C = x.shape
    y = _empty((NB, H, W, cp), device=x.device, dtype=torch.float32)
    stats = _empty((groups, MBSTD_STATS_STRIDE), device=x.device, dtype=torch.float32)
    _lib.call('pg_mbstd_fwd', _p(x), _p(y), _p(stats), groups, NB // groups, H * W, C, cp, _stream())
    return y, stats


def mbstd_tangent(x, tx, stats, cp):
    NB, H, W, C = x.shape
    groups = stats.shape[0]
    ty = torch.empty((NB, H, W, cp), device=x.device, dtype=torch.float32)
    tstats = torch.empty((groups, MBSTD_STATS_STRIDE), device=x.device, dtype=torch.float32)
    _lib.call('pg_mbstd_tangent', _p(x), _p(tx), _p(stats), _p(ty), _p(tstats), groups, NB // groups, H * W, C, cp, _stream())
    return ty, tstats


def mbstd_bwd(gy, x, stats, cp, apply_mask, mask_slope=0.2, tx=None, tstats=None, gy_first=None, out=None):
    NB, H, W, C = x.shape
    groups = stats.shape[0]
    gx = out if out is not None else torch.empty_like(x)
    _lib.call('pg_mbstd_bwd', _p(gy), _p(x), _p(stats), _p(tx), _p(tstats), _p(gy_first), _p(gx), groups,
              NB // groups, H * W, C, cp, 1 if apply_mask else 0, mask_slope, _stream())
    return gx


# exact-global mode under data parallelism (engine._mbstd_*: the partial rows / Gs sums travel between these calls)
def mbstd_stats(x, groups):
    NB, H, W, C = x.shape
    stats = torch.empty((groups, MBSTD_STATS_STRIDE), device=x.device, dtype=torch.float32)
    _lib.call('pg_mbstd_stats', _p(x), _p(stats), groups, NB // groups, H * W, C, _stream())
    return stats


def mbstd_write(x, stats, gathered, cp):
    """``gathered``: [nranks, groups, MBSTD_STATS_STRIDE] partial rows of all ranks (rank-major).  Returns (y, stats) with mu / sigma of the
    whole group (all shards) in stats[:, 0:2]."""
    NB, H, W, C = x.shape
    groups = stats.shape[0]
    y = torch.empty((NB, H, W, cp), device=x.device, dtype=torch.float32)
    _lib.call('pg_mbstd_write', _p(x), _p(y), _p(stats), _p(gathered), gathered.shape[0], groups, NB // groups, H * W, C, cp, _stream())
    return y, stats


def mbstd_tangent_stats(x, tx, stats):
    NB, H, W, C = x.shape
    groups = stats.shape[0]
    tstats = torch.empty((groups, MBSTD_STATS_STRIDE), device=x.device, dtype=torch.float32)
    _lib.call('pg_mbstd_tangent_stats', _p(x), _p(tx), _p(stats), _p(tstats), groups, NB // groups, H * W, C, _stream())
    return tstats


def mbstd_tangent_write(tx, tstats, gathered, stats, cp):
    NB, H, W, C = tx.shape
    groups = stats.shape[0]
    ty = torch.empty((NB, H, W, cp), device=tx.device, dtype=torch.float32)
    _lib.call('pg_mbstd_tangent_write', _p(tx), _p(ty), _p(tstats), _p(stats), _p(gathered), gathered.shape[0], groups, NB // groups, H * W, C, cp,
              _stream())
    return ty, tstats


def mbstd_gsum(gy, gy_first, groups, shape, cp):
    """[groups, 2]: this shard's sums of the stddev channel of ``gy`` / ``gy_first`` ([NB,H,W,cp]; either may be None)."""
    NB, H, W, C = shape
    ref = gy if gy is not None else gy_first
    out = torch.zeros((groups, 2), device=ref.device, dtype=torch.float32)
    _lib.call('pg_mbstd_gsum', _p(gy), _p(gy_first), _p(out), groups, NB // groups, H * W, C, cp, _stream())
    return out


def mbstd_bwd_global(gy, x, stats, cp, apply_mask, gsums, nranks, mask_slope=0.2, tx=None, tstats=None, gy_first=None, out=None):
    NB, H, W, C = x.shape
    groups = stats.shape[0]
    gx = out if out is not None else torch.empty_like(x)
    _lib.call('pg_mbstd_bwd_global', _p(gy), _p(x), _p(stats), _p(tx), _p(tstats), _p(gy_first), _p(gx), _p(gsums), nranks, groups,
              NB // groups, H * W, C, cp, 1 if apply_mask else 0, mask_slope, _stream())
    return gx


# ------------------------------------------------------------------------------------- linear
def linear1_fwd(h, w, b):
    N, C = h.shape[0], h.numel() // h.shape[0]
    s = _empty((N,), device=h.device, dtype=torch.float32)
    _lib.call('pg_linear1_fwd', _p(h), _p(w), _p(b), _p(s), N, C, _stream())
    return s


def linear1_bwd_data(gs, w, mask, shape, mask_slope=0.2):
    N = gs.shape[0]
    C = w.numel()
    gh = torch.empty(shape, device=gs.device, dtype=torch.float32)
    _lib.call('pg_linear1_bwd_data', _p(gs), _p(w), _p(mask), _p(gh), N, C, mask_slope, _stream())
    return gh


def linear1_wgrad(gs, h, dw, db):
    N = gs.shape[0]
    C = dw.numel()
    _lib.call('pg_linear1_wgrad', _p(gs), _p(h), _p(dw), _p(db), N, C, _stream())


# ------------------------------------------------------------------------------------ WGAN-GP
def gp_mix(real, fake, m, out=None):
    N = real.shape[0]
    E = real.numel() // N
    if out is None:
        out = torch.empty_like(real)
    _lib.call('pg_gp_mix', _p(real), _p(fake), _p(m), _p(out), N, E, _stream())
    return out


def row_sumsq(g):
    N = g.shape[0]
    E = g.numel() // N
    ss = torch.empty((N,), device=g.device, dtype=torch.float32)
    zero_(ss)
    _lib.call('pg_row_sumsq', _p(g), _p(ss), N, E, _stream())
    return ss


def gp_seed(g, ss, lam, target, inv_n):
    N = g.shape[0]
    E = g.numel() // N
    gp = torch.empty((N,), device=g.device, dtype=torch.float32)
    u = torch.empty_like(g)
    _lib.call('pg_gp_seed', _p(g), _p(ss), _p(gp), _p(u), N, E, lam, target, inv_n, _stream())
    return gp, u


def d_loss(scores, gp, N, eps):
    dev = scores.device
    out = torch.empty((1 + 2 * N,), device=dev, dtype=torch.float32)     # one buffer: a replayed step hands out ONE copy of it (plans.d_step)
    d_cost, d_real_loss, d_fake_loss = out[0], out[1:1 + N].view(N, 1), out[1 + N:].view(N, 1)
    gscore = torch.empty((3 * N,), device=dev, dtype=torch.float32)
    _lib.call('pg_d_loss', _p(scores), _p(gp), _p(d_cost), _p(d_real_loss), _p(d_fake_loss), _p(gscore), N, eps, _stream())
    return d_cost, d_real_loss, d_fake_loss, gscore


def g_loss(scores):
    N = scores.shape[0]
    g_cost = torch.empty((), device=scores.device, dtype=torch.float32)
    gscore = torch.empty((N,), device=scores.device, dtype=torch.float32)
    _lib.call('pg_g_loss', _p(scores), _p(g_cost), _p(gscore), N, _stream())
    return g_cost, gscore


# ------------------------------------------------------------------- selectable objectives (include/pggan_hip_gan.h)
# every #define PG_GAN_<KIND> of include/pggan_hip_gan.h, in the header's order: 'wgan', 'logistic', 'hinge', 'lsgan' -> the kernels' number
GAN_KINDS = {name[len('PG_GAN_'):].lower(): value for name, value in _lib.GAN_CONSTANTS.items() if name.startswith('PG_GAN_')}


def gan_d_loss(scores, pen, N, kind, drift):
    """``d_loss`` for any objective: ``scores`` [2N] or [3N] = [real | fake | (mixed)], ``pen`` [N] or None, ``kind`` a key of
    ``GAN_KINDS`` -> (d_cost, R [N,1], F [N,1], gscore of the length of ``scores``); the first three are views of one buffer."""
    dev = scores.device
    groups = scores.numel() // N
    out = torch.empty((1 + 2 * N,), device=dev, dtype=torch.float32)     # one buffer, as ``d_loss`` hands them out
    d_cost, d_real_loss, d_fake_loss = out[0], out[1:1 + N].view(N, 1), out[1 + N:].view(N, 1)
    gscore = torch.empty((groups * N,), device=dev, dtype=torch.float32)
    _lib.call('pg_gan_d_loss', _p(scores), _p(pen), _p(d_cost), _p(d_real_loss), _p(d_fake_loss), _p(gscore), N, groups,
              GAN_KINDS[kind], drift, _stream())
    return d_cost, d_real_loss, d_fake_loss, gscore


def gan_g_loss(scores, kind):
    N = scores.shape[0]
    g_cost = torch.empty((), device=scores.device, dtype=torch.float32)
    gscore = torch.empty((N,), device=scores.device, dtype=torch.float32)
    _lib.call('pg_gan_g_loss', _p(scores), _p(g_cost), _p(gscore), N, GAN_KINDS[kind], _stream())
    return g_cost, gscore


def r1_seed(g, ss, gamma, inv_n):
    """The R1 penalty per sample ``(gamma / 2) ss`` and its tangent seed ``(inv_n gamma) g`` (``gp_seed``'s place in the D step)."""
    N = g.shape[0]
    E = g.numel() // N
    pen = torch.empty((N,), device=g.device, dtype=torch.float32)
    u = torch.empty_like(g)
    _lib.call('pg_r1_seed', _p(g), _p(ss), _p(pen), _p(u), N, E, gamma, inv_n, _stream())
    return pen, u


# --------------------------------------------------------------------------------------- misc
def adam(p, g, m, v, lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale=1.0):
    _lib.call('pg_adam', _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale, _stream())


def ema(avg, p, beta):
    """avg += (1 - beta) * (p - avg) over two flat fp32 device tensors of one length (pg_ema_f32: the smoothed generator's weights)."""
    if avg.numel() != p.numel():
        raise ValueError('ema: %d averaged elements for %d parameters' % (avg.numel(), p.numel()))
    _lib.call('pg_ema_f32', _p(avg), _p(p), avg.numel(), beta, _stream())


def uniform_(t, seed, offset):
    """Fill the fp32 device tensor with U[0,1) draws: element i = Philox4x32-10(seed, offset, i) (wgan_gp_loss.py:15-17)."""
    require_gpu()
    _lib.call('pg_uniform_f32', _p(t), t.numel(), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _stream())
    return t


def zero_(t):
    _lib.call('pg_zero', _p(t), t.numel() * 4, _stream())
    return t


# ------------------------------------------------------------------------- input / output steps
def real_prepare_u8(x_u8, alpha, range_in=(0, 255), range_out=(-1, 1)):
    """uint8 device batch [N,C,H,W] -> faded + range-adjusted fp32 batch (dataset.py:54-67 on the device)."""
    if not x_u8.is_cuda or x_u8.dtype != torch.uint8 or not x_u8.is_contiguous():
        raise ValueError('expected a contiguous uint8 device tensor')
    N, C, H, W = x_u8.shape
    out = torch.empty((N, C, H, W), device=x_u8.device, dtype=torch.float32)
    _lib.call('pg_real_prepare_u8', x_u8.data_ptr(), _p(out), N * C, H, W, float(alpha), float(range_in[0]),
              float(range_in[1]), float(range_out[0]), float(range_out[1]), _stream())
    return out


SOUND_MODES = {'abslog': _C['PG_SOUND_ABSLOG'], 'reallog': _C['PG_SOUND_REALLOG']}


def spectrogram_u8(signal, n_fft, hop_length, max_out=255.0, img_mode='abslog'):
    """fp32 device waveform [nsamp] or [nsamp, channels] -> uint8 image (SoundImageDataset.load_file, dataset.py:285-300):
    'abslog' / 'reallog' spectrogram [1, n_fft/2, n_fft/2], or 'raw' [1, 2^s, 2^s] with 2^s = the largest power of two
    <= sqrt(nsamp) (dataset.py:289-291)."""
    require_gpu()
    if not signal.is_cuda or signal.dtype != torch.float32 or not signal.is_contiguous() or signal.dim() not in (1, 2):
        raise ValueError('expected a contiguous float32 device tensor [nsamp] or [nsamp, channels]')
    nsamp = signal.shape[0]
    ch = 1 if signal.dim() == 1 else signal.shape[1]
    if img_mode == 'raw':
        side = 1
        while (2 * side) * (2 * side) <= nsamp:
            side *= 2
        mag = torch.empty((side, side), device=signal.device, dtype=torch.float32)
        _lib.call('pg_mono_f32', _p(signal), nsamp, ch, _p(mag), side * side, _stream())
    else:
        if img_mode not in SOUND_MODES:
            raise ValueError("img_mode must be 'abslog', 'reallog' or 'raw' (got %r)" % (img_mode,))
        side = n_fft // 2
        if 1 + nsamp // hop_length < side:
            raise ValueError('%d samples give %d frames, the %dx%d image needs %d' % (nsamp, 1 + nsamp // hop_length, side, side, side))
        mag = torch.empty((side, side), device=signal.device, dtype=torch.float32)
        _lib.call('pg_stft_image', _p(signal), nsamp, ch, _p(mag), n_fft, hop_length, side, side, SOUND_MODES[img_mode], _stream())
    lohi = torch.empty(2, device=signal.device, dtype=torch.float32)
    _lib.call('pg_minmax_f32', _p(mag), mag.numel(), _p(lohi), _stream())
    out = torch.empty((1, side, side), device=signal.device, dtype=torch.uint8)
    _lib.call('pg_stretch_to_u8', _p(mag), out.data_ptr(), mag.numel(), _p(lohi), float(max_out), _stream())
    return out


def image_grid_u8(images, drange=(-1, 1), up=1):
    """fp32 device images [n,C,h,w] -> uint8 HWC grid (output_postprocess.py:35-62 up to the PIL hand-off)."""
    n, C, h, w = images.shape
    gw = 1
    while gw * gw < n:
        gw += 1
    gh = (n - 1) // gw + 1
    grid = torch.empty((gh * h * up, gw * w * up, C), device=images.device, dtype=torch.uint8)
    _lib.call('pg_image_grid_u8', _p(images), grid.data_ptr(), n, C, h, w, up, float(drange[0]), float(drange[1]), _stream())
    return grid


def pyramid_level_u8(batch_u8, depthdiff, range_in=(0, 255)):
    """uint8 device batch [..., H, W] -> the pyramid level ``depthdiff`` below it (dataset.py:243-250)."""
    require_gpu()
    if batch_u8.dtype != torch.uint8 or not batch_u8.is_cuda:
        raise RuntimeError('pyramid_level_u8 expects a uint8 tensor on the device')
    x = batch_u8.contiguous()
    H, W = x.shape[-2], x.shape[-1]
    st = 2 ** int(depthdiff)
    out = torch.empty(tuple(x.shape[:-2]) + (H // st, W // st), device=x.device, dtype=torch.uint8)
    _lib.call('pg_pyramid_level_u8', x.data_ptr(), out.data_ptr(), x.numel() // (H * W), H, W, int(depthdiff),
              float(range_in[0]), float(range_in[1]), _stream())
    return out


def _batch_operands(where, device, idx, pos, flip, C, S, depthdiff, alloc=True):
    """What ``real_batch_u8`` and ``crop_batch_u8`` share: the checks of the per-item tensors ``idx``, ``pos`` (None for a stack) and
    ``flip`` against the ``device`` of the ``where`` ('stack', 'level'), and the fp32 output [n,C,r,r], r = S >> depthdiff (not with
    ``alloc=False``: the callee allocates).  Returns (n, out)."""
    for name, t in (('idx', idx),) if pos is None else (('idx', idx), ('pos', pos)):
        if not torch.is_tensor(t) or t.device != device or t.dtype != torch.int64 or not t.is_contiguous() or t.dim() != 1 or t.numel() < 1:
            raise ValueError('%s: expected a contiguous, non-empty int64 tensor [n] on the device of the %s' % (name, where))
    n = idx.numel()
    if pos is not None and pos.numel() != n:
        raise ValueError('idx holds %d strips, pos %d start columns' % (n, pos.numel()))
    if flip is not None and (not torch.is_tensor(flip) or flip.device != device or flip.dtype != torch.uint8
                             or not flip.is_contiguous() or tuple(flip.shape) != (n,)):
        raise ValueError('flip: expected None or a contiguous uint8 tensor [%d] on the device of the %s' % (n, where))
    if not alloc:
        return n, None
    r = S >> depthdiff if 0 <= depthdiff < 31 else 0
    return n, torch.empty((n, C, r, r), device=device, dtype=torch.float32)


def real_batch_u8(stack_u8, idx, flip=None, depthdiff=0, alpha=1.0, range_in=(0, 255), range_out=(-1, 1), check=False):
    """uint8 device stack [M,C,S,S] -> fp32 batch [n,C,r,r], r = S >> depthdiff, in one launch (pg_real_batch_u8, csrc/real_batch.hip):
    image ``idx[j]`` (int64 device tensor [n]), its pyramid level (``pyramid_level_u8``), mirrored where ``flip[j] != 0`` (uint8 device
    tensor [n] or None), faded and range-adjusted (``real_prepare_u8``).  C = 2 (the 'magif' stacks) goes through pg_real_batch_2ch_u8 of
    include/pggan_hip_phase.h: the same kernels.  The device does not check ``idx``: ``check=True`` reads its
    minimum and maximum back (a host synchronisation) and raises IndexError for a value outside [0, M)."""
    require_gpu()
    if not torch.is_tensor(stack_u8) or not stack_u8.is_cuda or stack_u8.dtype != torch.uint8 or not stack_u8.is_contiguous() or stack_u8.dim() != 4:
        raise ValueError('expected a contiguous uint8 device stack [M,C,S,S]')
    M, C, S, S2 = stack_u8.shape
    if S != S2 or M < 1:
        raise ValueError('expected at least one square image, got a stack of shape %s' % (tuple(stack_u8.shape),))
    depthdiff = int(depthdiff)
    n, out = _batch_operands('stack', stack_u8.device, idx, None, flip, C, S, depthdiff, C != 2)
    if check:
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= M:
            raise IndexError('idx holds values in [%d, %d] for a stack of %d images' % (lo, hi, M))
    if C == 2:                                                   # pg_real_batch_u8 takes C in {1, 3}; two channels are an addition
        from . import phase
        return phase.real_batch_2ch_u8(stack_u8, idx, flip, depthdiff, alpha, range_in, range_out)
    _lib.call('pg_real_batch_u8', stack_u8.data_ptr(), M, C, S, depthdiff, idx.data_ptr(), None if flip is None else flip.data_ptr(), n,
              out.data_ptr(), float(alpha), float(range_in[0]), float(range_in[1]), float(range_out[0]), float(range_out[1]), _stream())
    return out


CROP = {name[len('PG_CROP_'):]: value for name, value in _lib.CROP_CONSTANTS.items() if name.startswith('PG_CROP_')}   # the addition's own table
CROP_TABLE_WORDS, CROP_PITCH_ALIGN = CROP['TABLE_WORDS'], CROP['PITCH_ALIGN']


def crop_batch_u8(level, idx, pos, flip=None, shift=0, depthdiff=0, alpha=1.0, range_in=(0, 255), range_out=(-1, 1), check=False):
    """One stored level of uint8 device strips (``dataset.StripLevel``: the flat ``buffer``, its ``table`` [M,3] int64 of (byte offset,
    row pitch, columns), ``C`` and the rows ``S``) -> fp32 batch [n,C,r,r], r = S >> depthdiff, in one launch (pg_crop_batch_u8,
    csrc/real_batch.hip): image j is the window of columns [u, u + S), u = pos[j] >> shift, of strip ``idx[j]`` (int64 device tensors
    [n]), treated as ``real_batch_u8`` treats an image of a stack -- the same two kernels, instantiated for strips: pyramid level, mirror
    where ``flip[j] != 0``, fade, range -- and equal to it bit for bit on the materialised windows.  The device checks neither ``idx``
    nor ``pos``: ``check=True`` reads their extrema back (a host synchronisation) and raises IndexError for a strip outside [0, M) or a
    window that leaves its strip."""
    require_gpu()
    buf, table = level.buffer, level.table
    if not torch.is_tensor(buf) or not buf.is_cuda or buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.dim() != 1:
        raise ValueError('level.buffer: expected a contiguous flat uint8 device tensor')
    if (not torch.is_tensor(table) or table.device != buf.device or table.dtype != torch.int64 or not table.is_contiguous()
            or table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != CROP_TABLE_WORDS):
        raise ValueError('level.table: expected a contiguous int64 tensor [M,%d] on the device of the buffer' % CROP_TABLE_WORDS)
    M, C, S = table.shape[0], int(level.C), int(level.S)
    shift, depthdiff = int(shift), int(depthdiff)
    if pos is None:
        raise ValueError('pos: expected a contiguous, non-empty int64 tensor [n] on the device of the level')
    n, out = _batch_operands('level', buf.device, idx, pos, flip, C, S, depthdiff)
    if check:
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= M:
            raise IndexError('idx holds values in [%d, %d] for a level of %d strips' % (lo, hi, M))
        u = pos >> shift if 0 <= shift < 63 else pos
        over = u - (table[:, 2][idx] - S)                        # > 0: the window ends past the strip's last column
        lo, hi = int(u.min()), int(over.max())
        if lo < 0 or hi > 0:
            raise IndexError('pos: a window starts at column %d or ends %d columns past the end of its strip' % (lo, hi))
    _lib.call('pg_crop_batch_u8', buf.data_ptr(), table.data_ptr(), M, C, S, shift, depthdiff, idx.data_ptr(), pos.data_ptr(),
              None if flip is None else flip.data_ptr(), n, out.data_ptr(), float(alpha), float(range_in[0]), float(range_in[1]),
              float(range_out[0]), float(range_out[1]), _stream())
    return out


# ------------------------------------------------------------------------- sliced Wasserstein distance (csrc/swd.hip)
SWD_DESC = _C['PG_SWD_DESC']                                   # 3 channels x 7 x 7
SWD_REDUCE_BLOCKS = _C['PG_SWD_REDUCE_BLOCKS']
SWD_SORT_LDS_ROW = _C['PG_SWD_SORT_RUN']                       # the longest row one workgroup sorts in LDS ...
SWD_SORT_MERGE_RUN = _C['PG_SWD_SORT_RUN']                     # ... and the run length the global merge of a longer row starts from
SWD_SORT_MERGE_TILE = _C['PG_SWD_SORT_MERGE_TILE']             # outputs per workgroup of a merge pass
SWD_SORT_MAX_M = _C['PG_SWD_SORT_MAX_M']


def _f32_dev(t, what, ndim=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('%s: expected a contiguous float32 device tensor' % what)
    if ndim is not None and t.dim() != ndim:
        raise ValueError('%s: expected %d dimensions, got shape %s' % (what, ndim, tuple(t.shape)))
    return t


def lap_pyramid(x, min_size=16):
    """fp32 device batch [N,3,S,S] (S a power of two >= 16) -> Laplacian pyramid [S, S/2, ..., 16] (pg_lap_down / pg_lap_up_sub):
    level i = g_i - up(g_{i+1}), the last level is the Gaussian level itself."""
    _f32_dev(x, 'lap_pyramid', 4)
    N, C, S, W = x.shape
    if S != W or S < min_size or (S & (S - 1)) or N < 1 or C < 1:
        raise ValueError('lap_pyramid: expected [N,C,S,S] with S a power of two >= %d, got %s' % (min_size, tuple(x.shape)))
    s = _stream()
    gauss = [x]
    while gauss[-1].shape[-1] > min_size:
        g = gauss[-1]
        h = g.shape[-1] // 2
        out = torch.empty((N, C, h, h), device=x.device, dtype=torch.float32)
        _lib.call('pg_lap_down', _p(g), _p(out), N * C, g.shape[-1], s)
        gauss.append(out)
    levels = []
    for fine, coarse in zip(gauss[:-1], gauss[1:]):
        out = torch.empty_like(fine)
        _lib.call('pg_lap_up_sub', _p(fine), _p(coarse), _p(out), N * C, fine.shape[-1], s)
        levels.append(out)
    levels.append(gauss[-1])
    return levels


def swd_gather(level, centres, P, out, row_offset, check_range=True):
    """Rows ``row_offset .. row_offset + N*P`` of ``out`` [M,147] <- the 3x7x7 neighbourhoods of ``level`` [N,3,S,S] around
    ``centres`` (int32 device [N*P,2] of (x, y) in [3, S-4]); descriptor j belongs to image j // P.  A centre outside that range is
    a ValueError; the check reads the centres back (one synchronisation), so a caller that has validated them on the host, as
    ``metrics.SlicedWasserstein`` does where it draws them, passes ``check_range=False``."""
    _f32_dev(level, 'swd_gather level', 4)
    _f32_dev(out, 'swd_gather out', 2)
    N, C, S, W = level.shape
    P, row_offset = int(P), int(row_offset)
    if N < 1 or C != 3 or S != W or S < 7:
        raise ValueError('swd_gather: expected a level [N,3,S,S] with N >= 1 and S >= 7, got %s' % (tuple(level.shape),))
    if not torch.is_tensor(centres) or not centres.is_cuda or centres.dtype != torch.int32 or not centres.is_contiguous() \
            or P < 1 or tuple(centres.shape) != (N * P, 2):
        raise ValueError('swd_gather: expected contiguous int32 device centres [%d,2]' % (N * P))
    if out.shape[1] != SWD_DESC or row_offset < 0 or row_offset + N * P > out.shape[0]:
        raise ValueError('swd_gather: rows %d..%d do not fit out %s' % (row_offset, row_offset + N * P, tuple(out.shape)))
    if check_range:
        lo, hi = int(centres.min()), int(centres.max())
        if lo < 3 or hi > S - 4:
            raise ValueError('swd_gather: centres span %d..%d, outside [3, %d] of a %dx%d level' % (lo, hi, S - 4, S, S))
    _lib.call('pg_swd_gather', _p(level), centres.data_ptr(), _p(out), N * P, P, S, row_offset, out.shape[0], _stream())
    return out


def _swd_partials(device, per_block=1):
    return torch.empty(SWD_REDUCE_BLOCKS * per_block, device=device, dtype=torch.float64)


def swd_normalize_(desc):
    """In place: per channel, subtract the mean and divide by the population standard deviation over all rows of ``desc`` [M,147]."""
    _f32_dev(desc, 'swd_normalize_', 2)
    if desc.shape[1] != SWD_DESC or desc.shape[0] < 1:
        raise ValueError('swd_normalize_: expected [M,147] with M >= 1, got %s' % (tuple(desc.shape),))
    s = _stream()
    partials = _swd_partials(desc.device, 6)
    stats = torch.empty(6, device=desc.device, dtype=torch.float32)
    _lib.call('pg_swd_channel_stats', _p(desc), desc.shape[0], partials.data_ptr(), _p(stats), s)
    _lib.call('pg_swd_normalize', _p(desc), desc.shape[0], _p(stats), s)
    return desc


def swd_project(desc, dirs, out=None):
    """``desc`` [M,147] x ``dirs`` [147,K] -> [K,M]: every direction's projections are one contiguous row."""
    _f32_dev(desc, 'swd_project desc', 2)
    _f32_dev(dirs, 'swd_project dirs', 2)
    M, K = desc.shape[0], dirs.shape[1]
    if desc.shape[1] != SWD_DESC or dirs.shape[0] != SWD_DESC or M < 1 or K < 1:
        raise ValueError('swd_project: expected [M,147] and [147,K], got %s and %s' % (tuple(desc.shape), tuple(dirs.shape)))
    if out is None:
        out = torch.empty((K, M), device=desc.device, dtype=torch.float32)
    elif tuple(_f32_dev(out, 'swd_project out', 2).shape) != (K, M):
        raise ValueError('swd_project: out must be [%d,%d]' % (K, M))
    _lib.call('pg_swd_project', _p(desc), _p(dirs), _p(out), M, K, _stream())
    return out


# The same three steps for C = 1 .. 4 channels (include/pggan_hip_swd.h): descriptors of 49 C floats.  UNPINNED for C != 3: this
# project's extension of the paper's 7x7x3 descriptor.  C = 3 runs the kernels of the three wrappers above and gives their bits.
_SWD_C = {name[len('PG_SWD_'):]: value for name, value in _lib.SWD_CONSTANTS.items() if name.startswith('PG_SWD_')}   # the addition's own table
SWD_PATCH = _SWD_C['PATCH']                                    # 7 x 7: floats of one channel of a descriptor
SWD_MAX_CHANNELS = _SWD_C['MAX_CHANNELS']


def swd_channels(width, what='descriptor width'):
    """The channel count C of a descriptor of ``width`` = 49 C floats, C in 1 .. SWD_MAX_CHANNELS; anything else is a ValueError."""
    width = int(width)
    if width % SWD_PATCH or not 1 <= width // SWD_PATCH <= SWD_MAX_CHANNELS:
        raise ValueError('%s: %d is not %d * C for C in 1 .. %d' % (what, width, SWD_PATCH, SWD_MAX_CHANNELS))
    return width // SWD_PATCH


def swd_gather_c(level, centres, P, out, row_offset, check_range=True):
    """``swd_gather`` for a level [N,C,S,S] with C in 1 .. 4: rows ``row_offset .. row_offset + N*P`` of ``out`` [M,49*C] <- the Cx7x7
    neighbourhoods around ``centres``, rows in (channel, dy, dx) order.  The channel count is the level's; an ``out`` of another
    width is a ValueError."""
    _f32_dev(level, 'swd_gather_c level', 4)
    _f32_dev(out, 'swd_gather_c out', 2)
    N, C, S, W = level.shape
    P, row_offset = int(P), int(row_offset)
    if N < 1 or not 1 <= C <= SWD_MAX_CHANNELS or S != W or S < 7:
        raise ValueError('swd_gather_c: expected a level [N,C,S,S] with N >= 1, 1 <= C <= %d and S >= 7, got %s'
                         % (SWD_MAX_CHANNELS, tuple(level.shape)))
    if not torch.is_tensor(centres) or not centres.is_cuda or centres.dtype != torch.int32 or not centres.is_contiguous() \
            or P < 1 or tuple(centres.shape) != (N * P, 2):
        raise ValueError('swd_gather_c: expected contiguous int32 device centres [%d,2]' % (N * P))
    if out.shape[1] != SWD_PATCH * C or row_offset < 0 or row_offset + N * P > out.shape[0]:
        raise ValueError('swd_gather_c: rows %d..%d of %d floats do not fit out %s'
                         % (row_offset, row_offset + N * P, SWD_PATCH * C, tuple(out.shape)))
    if check_range:
        lo, hi = int(centres.min()), int(centres.max())
        if lo < 3 or hi > S - 4:
            raise ValueError('swd_gather_c: centres span %d..%d, outside [3, %d] of a %dx%d level' % (lo, hi, S - 4, S, S))
    _lib.call('pg_swd_gather_c', _p(level), centres.data_ptr(), _p(out), N * P, P, C, S, row_offset, out.shape[0], _stream())
    return out


def swd_normalize_c_(desc):
    """``swd_normalize_`` for ``desc`` [M,49*C], C in 1 .. 4 (from the width): every channel to zero mean and unit population
    standard deviation over all rows, in place."""
    _f32_dev(desc, 'swd_normalize_c_', 2)
    C = swd_channels(desc.shape[1], 'swd_normalize_c_')
    if desc.shape[0] < 1:
        raise ValueError('swd_normalize_c_: expected [M,%d] with M >= 1, got %s' % (desc.shape[1], tuple(desc.shape)))
    s = _stream()
    partials = _swd_partials(desc.device, 2 * C)
    stats = torch.empty(2 * C, device=desc.device, dtype=torch.float32)
    _lib.call('pg_swd_channel_stats_c', _p(desc), desc.shape[0], C, partials.data_ptr(), _p(stats), s)
    _lib.call('pg_swd_normalize_c', _p(desc), desc.shape[0], C, _p(stats), s)
    return desc


def swd_project_c(desc, dirs, out=None):
    """``swd_project`` for ``desc`` [M,49*C] x ``dirs`` [49*C,K] -> [K,M], C in 1 .. 4 (from the widths, which must agree)."""
    _f32_dev(desc, 'swd_project_c desc', 2)
    _f32_dev(dirs, 'swd_project_c dirs', 2)
    M, K = desc.shape[0], dirs.shape[1]
    C = swd_channels(desc.shape[1], 'swd_project_c desc')
    if dirs.shape[0] != desc.shape[1] or M < 1 or K < 1:
        raise ValueError('swd_project_c: expected [M,%d] and [%d,K], got %s and %s'
                         % (desc.shape[1], desc.shape[1], tuple(desc.shape), tuple(dirs.shape)))
    if out is None:
        out = torch.empty((K, M), device=desc.device, dtype=torch.float32)
    elif tuple(_f32_dev(out, 'swd_project_c out', 2).shape) != (K, M):
        raise ValueError('swd_project_c: out must be [%d,%d]' % (K, M))
    _lib.call('pg_swd_project_c', _p(desc), _p(dirs), _p(out), M, C, K, _stream())
    return out


def swd_sort_rows_(buf, tmp=None):
    """Sort every row of ``buf`` [K,M] ascending, in place.  Rows longer than SWD_SORT_LDS_ROW need a scratch of buf's shape
    (``tmp``; allocated when not given)."""
    _f32_dev(buf, 'swd_sort_rows_', 2)
    K, M = buf.shape
    if K < 1 or K > 65535 or M < 1 or M > SWD_SORT_MAX_M:
        raise ValueError('swd_sort_rows_: expected [K,M] with 1 <= K <= 65535 and 1 <= M <= 2^22, got %s' % (tuple(buf.shape),))
    if M > SWD_SORT_LDS_ROW:
        if tmp is None:
            tmp = torch.empty_like(buf)
        elif _f32_dev(tmp, 'swd_sort_rows_ tmp').numel() < buf.numel() or tmp.data_ptr() == buf.data_ptr():
            raise ValueError('swd_sort_rows_: tmp must be a separate buffer of at least %d floats' % buf.numel())
    _lib.call('pg_swd_sort_rows', _p(buf), _p(tmp) if M > SWD_SORT_LDS_ROW else None, K, M, _stream())
    return buf


def swd_l1(a, b):
    """mean |a - b| over two equal-shaped fp32 device tensors -> 0-dim device tensor."""
    _f32_dev(a, 'swd_l1 a')
    _f32_dev(b, 'swd_l1 b')
    if a.shape != b.shape or a.numel() < 1:
        raise ValueError('swd_l1: expected two equal, non-empty shapes, got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    partials = _swd_partials(a.device)
    out = torch.empty((), device=a.device, dtype=torch.float32)
    _lib.call('pg_swd_l1', _p(a), _p(b), a.numel(), partials.data_ptr(), _p(out), _stream())
    return out


# ------------------------------------------------------------------------- multi-scale SSIM between image pairs (csrc/msssim.hip)
MSSSIM_TILE = _C['PG_MSSSIM_TILE']                             # outputs (and pixels) per workgroup side
MSSSIM_WINDOW = 11                 # taps of the Gaussian window; a scale's side is at least 16 so that the window always fits whole
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli & Bovik 2003
assert len(MSSSIM_WEIGHTS) == _C['PG_MSSSIM_MAX_SCALES']
MSSSIM_MODES = {'as_is': 0, 'range': 1, 'quantize': 2}


def msssim_scales(resolution):
    """Host function: (sides, weights) of the scales of a ``resolution`` x ``resolution`` image.  S = min(5, log2(R) - 3) scales of
    side R, R/2, ... (each >= 16); the weights are the first S published ones over their sum."""
    resolution = int(resolution)
    if resolution < 16 or resolution & (resolution - 1):
        raise ValueError('resolution must be a power of two >= 16, got %r' % (resolution,))
    S = min(len(MSSSIM_WEIGHTS), resolution.bit_length() - 4)
    total = sum(MSSSIM_WEIGHTS[:S])
    return [resolution >> s for s in range(S)], [w / total for w in MSSSIM_WEIGHTS[:S]]


def _msssim_tiles(side):
    return (side - (MSSSIM_WINDOW - 1) + MSSSIM_TILE - 1) // MSSSIM_TILE


def _msssim_check(a, b, what):
    for t, name in ((a, 'a'), (b, 'b')):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('%s %s: expected a contiguous float32 device tensor' % (what, name))
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError('%s: expected two equal shapes [n,C,R,R], got %s and %s' % (what, tuple(a.shape), tuple(b.shape)))
    n, C, R, W = a.shape
    if n < 1 or C not in (1, 3) or R != W or R < 16 or (R & (R - 1)):
        raise ValueError('%s: expected [n,C,R,R] with n >= 1, C in (1, 3) and R a power of two >= 16, got %s' % (what, tuple(a.shape)))
    return n, C, R


class MSSSIMScratch(object):
    """Work buffers of ``msssim_pairs`` for batches of up to ``n`` pairs ``[n,C,R,R]``: per scale below the finest the pooled images of
    a and of b (``pooled[s - 1] = (a_s, b_s)``, fp32 ``[n,C,R >> s,R >> s]``) and the per-workgroup partial sums of every scale
    (``partials[s]``, fp64 ``[n * C * tiles_s^2, 2]`` of (sum of ssim, sum of cs))."""

    def __init__(self, n, C, R, device):
        self.n, self.C, self.R = int(n), int(C), int(R)
        self.sides, self.weights = msssim_scales(R)
        self.pooled = [tuple(torch.empty((self.n, self.C, s, s), device=device, dtype=torch.float32) for _ in range(2))
                       for s in self.sides[1:]]
        self.partial_rows = [self.C * _msssim_tiles(s) ** 2 for s in self.sides]          # per pair
        self._partials = torch.empty((self.n * sum(self.partial_rows), 2), device=device, dtype=torch.float64)

    def partials(self, n):
        """The blocks of the scales for a batch of ``n`` pairs, one after the other from the start of the buffer (what pg_msssim_finish reads)."""
        out, start = [], 0
        for rows in self.partial_rows:
            out.append(self._partials[start:start + n * rows])
            start += n * rows
        return out


def msssim_scale(a, b, pool_a, pool_b, partials, mode, drange=(-1, 1)):
    """One scale (pg_msssim_scale) of the planes ``a``, ``b`` [n,C,s,s]: fills ``partials`` [n*C*tiles^2, 2] and, when given, the
    pooled images [n,C,s/2,s/2].  ``mode``: 'quantize' / 'range' (the finest scale, with / without rounding and clipping) or 'as_is'."""
    n, C, side, _ = a.shape
    _lib.call('pg_msssim_scale', _p(a), _p(b), _p(pool_a), _p(pool_b), partials.data_ptr(), n * C, side, MSSSIM_MODES[mode],
              float(drange[0]), float(drange[1]), _stream())


def msssim_pairs(a, b, drange=(-1, 1), quantize=True, out=None, scratch=None):
    """MS-SSIM of the pairs ``(a[i], b[i])`` of two fp32 device batches [n,C,R,R], C in (1, 3), R a power of two >= 16 (DESIGN.md
    section 7; one launch per scale plus one).  Returns ``(values [n], terms [n,S])``, fp64 device tensors: ``terms`` holds the mean
    contrast-structure term of every scale below the last and the mean ssim of the last, ``values`` the weighted product of the terms
    clamped at 0.  ``quantize``: round and clip to the 0..255 levels of the saved image first (``ops.image_grid_u8``'s arithmetic);
    False maps ``drange`` to [0, 255] only.  ``out``: a ``(values, terms)`` pair to write into; ``scratch``: an ``MSSSIMScratch`` of
    at least this batch (allocated when not given; ``scratch.pooled`` holds the pooled images afterwards).  No host synchronisation."""
    n, C, R = _msssim_check(a, b, 'msssim_pairs')
    lo, hi = float(drange[0]), float(drange[1])
    if not hi > lo:
        raise ValueError('msssim_pairs: drange must be (lo, hi) with hi > lo, got %r' % (drange,))
    if scratch is None:
        scratch = MSSSIMScratch(n, C, R, a.device)
    elif scratch.n < n or (scratch.C, scratch.R) != (C, R) or scratch._partials.device != a.device:
        raise ValueError('msssim_pairs: scratch is for up to %d pairs [%d,%d,%d] on %s' % (scratch.n, scratch.C, scratch.R, scratch.R,
                                                                                          scratch._partials.device))
    S = len(scratch.sides)
    if out is None:
        values = torch.empty(n, device=a.device, dtype=torch.float64)
        terms = torch.empty((n, S), device=a.device, dtype=torch.float64)
    else:
        values, terms = out
        for t, shape in ((values, (n,)), (terms, (n, S))):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError('msssim_pairs: out must be contiguous float64 device tensors [%d] and [%d,%d]' % (n, n, S))
    partials = scratch.partials(n)
    cur_a, cur_b = a, b
    for s in range(S):
        nxt = (None, None) if s == S - 1 else tuple(t[:n] for t in scratch.pooled[s])
        msssim_scale(cur_a, cur_b, nxt[0], nxt[1], partials[s], ('quantize' if quantize else 'range') if s == 0 else 'as_is', (lo, hi))
        cur_a, cur_b = nxt
    _lib.call('pg_msssim_finish', partials[0].data_ptr(), values.data_ptr(), terms.data_ptr(), n, C, R, _stream())
    return values, terms


# ------------------------------------------------------------------------- nearest training images (csrc/nn_search.hip)
NN_MAX_QUERIES = _C['PG_NN_MAX_QUERIES']                       # queries of one pass over the stack; more are split into several passes
NN_MAX_TOPK = _C['PG_NN_MAX_TOPK']


def _u8_images(t, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or t.dim() != 4 or t.shape[0] < 1:
        raise ValueError('%s: expected a contiguous, non-empty uint8 device tensor [n,C,r,r]' % what)


def _image_bytes(images_u8, who):
    """(n, D) of a checked uint8 image tensor [n,C,r,r]: D = C r^2 bytes per image, a multiple of 16 (the kernels load 16 bytes at a
    time); ``who`` is the refusing call."""
    n = images_u8.shape[0]
    D = images_u8.numel() // n
    if D % 16:
        raise ValueError('%s: an image of %d bytes (a multiple of 16 is required)' % (who, D))
    return n, D


def _dev_tensor(t, dtype, shape, device, what):
    """``t`` when it is a contiguous ``dtype`` tensor of ``shape`` on ``device``, where the call's images are; ``what`` = 'call: argument'."""
    if not torch.is_tensor(t) or t.device != device or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be a contiguous %s tensor %s on the device of the other operands (%s)'
                         % (what, str(dtype).replace('torch.', ''), list(shape), device))
    return t


def quantize_u8(images, drange=(-1, 1)):
    """fp32 device images [n,C,r,r] in ``drange`` -> the uint8 levels of the saved image in the same layout (pg_quantize_u8):
    ``(x - lo) * (255 / (hi - lo))`` in fp32 with one rounding per operation, round half to even, clip to [0, 255] -- the arithmetic of
    ``image_grid_u8`` and ``msssim_pairs``."""
    if not torch.is_tensor(images) or not images.is_cuda or images.dtype != torch.float32 or not images.is_contiguous() or images.numel() < 1:
        raise ValueError('quantize_u8: expected a contiguous, non-empty float32 device tensor')
    lo, hi = float(drange[0]), float(drange[1])
    if not hi > lo:
        raise ValueError('quantize_u8: drange must be (lo, hi) with hi > lo, got %r' % (drange,))
    require_gpu()
    out = torch.empty(tuple(images.shape), device=images.device, dtype=torch.uint8)
    _lib.call('pg_quantize_u8', images.data_ptr(), out.data_ptr(), images.numel(), lo, hi, _stream())
    return out


def l2dist_u8(stack_u8, queries_u8, out=None):
    """Exact squared L2 distances between uint8 device images: ``stack_u8`` [M,C,r,r], ``queries_u8`` [K,C,r,r] -> int64 [K,M],
    ``out[k, m] = sum_d (stack[m, d] - queries[k, d])^2`` (pg_l2dist_u8, on the int8 MFMA).  Every pass reads the stack once for up to
    ``NN_MAX_QUERIES`` queries; more queries take ceil(K / NN_MAX_QUERIES) passes, each into its rows of ``out``.  ``out``: a
    contiguous int64 device tensor [K,M] to write into.  No host synchronisation."""
    _u8_images(stack_u8, 'l2dist_u8 stack')
    _u8_images(queries_u8, 'l2dist_u8 queries')
    if queries_u8.device != stack_u8.device or tuple(queries_u8.shape[1:]) != tuple(stack_u8.shape[1:]):
        raise ValueError('l2dist_u8: queries %s on %s do not match the stack %s on %s'
                         % (tuple(queries_u8.shape), queries_u8.device, tuple(stack_u8.shape), stack_u8.device))
    (M, D), K = _image_bytes(stack_u8, 'l2dist_u8'), queries_u8.shape[0]
    if out is None:
        out = torch.empty((K, M), device=stack_u8.device, dtype=torch.int64)
    else:
        _dev_tensor(out, torch.int64, (K, M), stack_u8.device, 'l2dist_u8: out')
    require_gpu()
    s = _stream()
    for k0 in range(0, K, NN_MAX_QUERIES):
        k1 = min(K, k0 + NN_MAX_QUERIES)
        _lib.call('pg_l2dist_u8', stack_u8.data_ptr(), M, queries_u8[k0:k1].data_ptr(), k1 - k0, D, out[k0:k1].data_ptr(), s)
    return out


def topk_smallest_i64(dist, k):
    """int64 device tensor [K,M] -> (values [K,k], indices [K,k]) int64: the ``k`` smallest of every row, ascending by (value, index) --
    of equal values the lower index comes first (pg_topk_smallest_i64).  1 <= k <= min(M, NN_MAX_TOPK)."""
    if not torch.is_tensor(dist) or not dist.is_cuda or dist.dtype != torch.int64 or not dist.is_contiguous() or dist.dim() != 2 or dist.numel() < 1:
        raise ValueError('topk_smallest_i64: expected a contiguous, non-empty int64 device tensor [K,M]')
    K, M = dist.shape
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= min(M, NN_MAX_TOPK):
        raise ValueError('topk_smallest_i64: k = %r for rows of %d (1 <= k <= min(M, %d))' % (k, M, NN_MAX_TOPK))
    k = int(k)
    require_gpu()
    values = torch.empty((K, k), device=dist.device, dtype=torch.int64)
    indices = torch.empty((K, k), device=dist.device, dtype=torch.int64)
    _lib.call('pg_topk_smallest_i64', dist.data_ptr(), K, M, k, values.data_ptr(), indices.data_ptr(), _stream())
    return values, indices


def nn_search_u8(stack_u8, queries_u8, k=1):
    """The ``k`` nearest stack images of every query by exact squared L2 distance over the uint8 levels: ``(sqdist [K,k], index [K,k])``,
    int64 device tensors, ascending by (distance, index).  ``l2dist_u8`` followed by ``topk_smallest_i64``; ``k > M`` is a ValueError."""
    _u8_images(stack_u8, 'nn_search_u8 stack')
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= min(stack_u8.shape[0], NN_MAX_TOPK):
        raise ValueError('nn_search_u8: k = %r for a stack of %d images (1 <= k <= min(M, %d))' % (k, stack_u8.shape[0], NN_MAX_TOPK))
    return topk_smallest_i64(l2dist_u8(stack_u8, queries_u8), k)


# ------------------------------------------------------------------------- k-NN balls: precision / recall / density / coverage (csrc/prd.hip)
PRD = {name[len('PG_PRD_'):]: value for name, value in _lib.PRD_CONSTANTS.items() if name.startswith('PG_PRD_')}   # the addition's own table
PRD_TILE = PRD['TILE']                                         # columns of one candidate block of pg_prd_kth_u8


def _prd_radii(rad, n, device, what):
    return None if rad is None else _dev_tensor(rad, torch.int64, (n,), device, 'prd_ball_u8: ' + what)


def prd_kth_u8(x_u8, k):
    """The k-NN radii of a set of uint8 device images ``x_u8`` [N,C,r,r]: int64 [N], ``rad[i]`` = the ``k``-th smallest of the exact
    squared L2 distances ``sum_d (x[i, d] - x[j, d])^2`` over j != i -- the exclusion is by index, a duplicate of image i elsewhere counts
    with distance 0.  pg_prd_kth_u8 leaves the ``k`` smallest of every block of ``PRD_TILE`` columns ([N, ceil(N / PRD_TILE), k] int64:
    nothing of size N x N exists), ``topk_smallest_i64`` takes the ``k``-th of those.  N >= k + 1, 1 <= k <= NN_MAX_TOPK.  No host
    synchronisation."""
    _u8_images(x_u8, 'prd_kth_u8')
    N = x_u8.shape[0]
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= min(N - 1, NN_MAX_TOPK):
        raise ValueError('prd_kth_u8: k = %r for %d images (1 <= k <= min(N - 1, %d))' % (k, N, NN_MAX_TOPK))
    _, D = _image_bytes(x_u8, 'prd_kth_u8')
    k = int(k)
    require_gpu()
    blocks = (N + PRD_TILE - 1) // PRD_TILE
    cand = torch.empty((N, blocks, k), device=x_u8.device, dtype=torch.int64)
    _lib.call('pg_prd_kth_u8', x_u8.data_ptr(), N, D, k, cand.data_ptr(), _stream())
    values, _ = topk_smallest_i64(cand.view(N, blocks * k), k)
    return values[:, k - 1].contiguous()


def prd_ball_u8(a_u8, b_u8, rad_a=None, rad_b=None):
    """One pass over the pairs (p, c) of uint8 device images ``a_u8`` [Na,C,r,r] and ``b_u8`` [Nb,C,r,r] (pg_prd_ball_u8), with
    ``d2 = sum_d (a[p, d] - b[c, d])^2`` exact: ``(a_cnt, a_hit, b_cnt, b_hit)``, int32 device tensors,
    ``a_cnt[p] = #{c : d2 <= rad_b[c]}``, ``b_hit[c] = #{p : d2 <= rad_b[c]}`` (None without ``rad_b``) and
    ``b_cnt[c] = #{p : d2 <= rad_a[p]}``, ``a_hit[p] = #{c : d2 <= rad_a[p]}`` (None without ``rad_a``).  ``rad_a`` [Na], ``rad_b`` [Nb]:
    contiguous int64 device tensors, at least one of them.  No distance is written; no host synchronisation."""
    _u8_images(a_u8, 'prd_ball_u8 a')
    _u8_images(b_u8, 'prd_ball_u8 b')
    if b_u8.device != a_u8.device or tuple(b_u8.shape[1:]) != tuple(a_u8.shape[1:]):
        raise ValueError('prd_ball_u8: b %s on %s does not match a %s on %s'
                         % (tuple(b_u8.shape), b_u8.device, tuple(a_u8.shape), a_u8.device))
    (Na, D), Nb = _image_bytes(a_u8, 'prd_ball_u8'), b_u8.shape[0]
    rad_a = _prd_radii(rad_a, Na, a_u8.device, 'rad_a')
    rad_b = _prd_radii(rad_b, Nb, a_u8.device, 'rad_b')
    if rad_a is None and rad_b is None:
        raise ValueError('prd_ball_u8: neither rad_a nor rad_b')
    require_gpu()
    a_cnt = b_hit = b_cnt = a_hit = None
    if rad_b is not None:
        a_cnt = torch.empty((Na,), device=a_u8.device, dtype=torch.int32)
        b_hit = torch.empty((Nb,), device=a_u8.device, dtype=torch.int32)
    if rad_a is not None:
        b_cnt = torch.empty((Nb,), device=a_u8.device, dtype=torch.int32)
        a_hit = torch.empty((Na,), device=a_u8.device, dtype=torch.int32)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.call('pg_prd_ball_u8', a_u8.data_ptr(), Na, b_u8.data_ptr(), Nb, D, ptr(rad_a), ptr(rad_b), ptr(a_cnt), ptr(a_hit), ptr(b_cnt),
              ptr(b_hit), _stream())
    return a_cnt, a_hit, b_cnt, b_hit


# ------------------------------------------------------------------------- random embedding and fp64 moments: the Frechet distance (csrc/embed.hip)
EMBED = {name[len('PG_'):]: value for name, value in _lib.EMBED_CONSTANTS.items()}   # the addition's own table
EMB_STEM_CH, EMB_MAX_C = EMBED['EMB_STEM_CH'], EMBED['EMB_MAX_C']
FD_SLICE, FD_TILE, FD_MIN_F, FD_MAX_F = EMBED['FD_SLICE'], EMBED['FD_TILE'], EMBED['FD_MIN_F'], EMBED['FD_MAX_F']


def _bf16_map(x, who):
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.bfloat16 or not x.is_contiguous() or x.dim() != 4 or x.numel() < 1:
        raise ValueError('%s: expected a contiguous, non-empty bfloat16 device tensor [N,H,W,Ch]' % who)
    return tuple(x.shape)


def emb_stem_u8_bf16(x_u8):
    """uint8 device images ``x_u8`` [M,C,H,W], 1 <= C <= ``EMB_MAX_C`` -> the bf16 NHWC input [M,H,W,``EMB_STEM_CH``] of the embedding's
    first 3x3 layer (pg_emb_stem_u8_bf16): ``rne_bf16((float(x) - 127.5f) / 127.5f)`` in channels 0 .. C - 1, zeros above."""
    _u8_images(x_u8, 'emb_stem_u8_bf16')
    M, C, H, W = x_u8.shape
    if not 1 <= C <= EMB_MAX_C:
        raise ValueError('emb_stem_u8_bf16: %d image channels (1 <= C <= %d)' % (C, EMB_MAX_C))
    require_gpu()
    y = torch.empty((M, H, W, EMB_STEM_CH), device=x_u8.device, dtype=torch.bfloat16)
    _lib.call('pg_emb_stem_u8_bf16', x_u8.data_ptr(), y.data_ptr(), M, C, H, W, _stream())
    return y


def emb_pool2_bf16(x):
    """bf16 device map ``x`` [N,H,W,Ch] (H, W even, Ch % 8 == 0) -> its 2x2 mean [N,H/2,W/2,Ch] in bf16 (pg_emb_pool2_bf16):
    ``rne_bf16(((a00 + a01) + (a10 + a11)) * 0.25f)`` in fp32, in that order."""
    N, H, W, Ch = _bf16_map(x, 'emb_pool2_bf16')
    if H % 2 or W % 2 or Ch % 8:
        raise ValueError('emb_pool2_bf16: a map %s (H and W even, Ch a multiple of 8)' % ((N, H, W, Ch),))
    require_gpu()
    y = torch.empty((N, H // 2, W // 2, Ch), device=x.device, dtype=torch.bfloat16)
    _lib.call('pg_emb_pool2_bf16', x.data_ptr(), y.data_ptr(), N, H, W, Ch, _stream())
    return y


def emb_gap_f32(x):
    """bf16 device map ``x`` [N,H,W,Ch] -> its mean over the pixels [N,Ch] in fp32 (pg_emb_gap_f32): the fp32 sum over (h, w) in
    ascending row-major order from 0, times ``1.0f / (H W)``."""
    N, H, W, Ch = _bf16_map(x, 'emb_gap_f32')
    require_gpu()
    f = torch.empty((N, Ch), device=x.device, dtype=torch.float32)
    _lib.call('pg_emb_gap_f32', x.data_ptr(), f.data_ptr(), N, H, W, Ch, _stream())
    return f


def fd_moments_scratch(M, F):
    """The fp64 values of scratch pg_fd_moments_f64 needs for [M,F] features: the column sums and the covariance tiles on or above the
    diagonal of every slice of ``FD_SLICE`` rows."""
    S, B = (M + FD_SLICE - 1) // FD_SLICE, (F + FD_TILE - 1) // FD_TILE
    return S * (F + B * (B + 1) // 2 * FD_TILE * FD_TILE)


def fd_moments_f64(x):
    """fp32 device features ``x`` [M,F] (M >= 2, F a multiple of 16, ``FD_MIN_F`` <= F <= ``FD_MAX_F``) -> ``(mean [F], cov [F,F])`` in
    fp64 (pg_fd_moments_f64): ``cov = sum_r (x_r - mean)(x_r - mean)^T / (M - 1)``, centred on the call's own mean, accumulated on the
    fp64 matrix cores in an order that depends on (M, F) alone; ``cov == cov.T`` bit for bit and two calls give the same bits.  The
    scratch is allocated here and every element of it is written.  No host synchronisation."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2:
        raise ValueError('fd_moments_f64: expected a contiguous float32 device tensor [M,F]')
    M, F = x.shape
    if M < 2 or F % 16 or not FD_MIN_F <= F <= FD_MAX_F:
        raise ValueError('fd_moments_f64: features [%d,%d] (M >= 2, F a multiple of 16, %d <= F <= %d)' % (M, F, FD_MIN_F, FD_MAX_F))
    require_gpu()
    mean = torch.empty((F,), device=x.device, dtype=torch.float64)
    cov = torch.empty((F, F), device=x.device, dtype=torch.float64)
    scratch = torch.empty((fd_moments_scratch(M, F),), device=x.device, dtype=torch.float64)
    _lib.call('pg_fd_moments_f64', x.data_ptr(), M, F, mean.data_ptr(), cov.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream())
    return mean, cov


# ------------------------------------------------------------------------- tile sums of the cubic kernel: the kernel distance (csrc/kid.hip)
KID = {name[len('PG_KID_'):]: value for name, value in _lib.KID_CONSTANTS.items()}   # the addition's own table
KID_TILE, KID_MIN_F, KID_MAX_F = KID['TILE'], KID['MIN_F'], KID['MAX_F']


def _kid_features(t, who):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2:
        raise ValueError('kid_tilesums_f64: expected %s as a contiguous float32 device tensor [rows,F]' % who)
    return t.shape


def kid_tilesums_f64(x, y=None, gamma=None, coef0=1.0, skip_diagonal=False, out=None):
    """fp32 device features ``x`` [M,F] and ``y`` [N,F] (None: y = x, the self form) -> fp64 ``[A,B]`` with A = ceil(M / ``KID_TILE``),
    B = ceil(N / ``KID_TILE``) (pg_kid_tilesums_f64): ``sums[a,b]`` = the sum of ``k(x_i, y_j) = (gamma x_i . y_j + coef0)^3`` over the
    pairs of tile (a, b) with i < M and j < N, without the pairs i == j when ``skip_diagonal`` (the self form only).  ``gamma`` None:
    ``1.0 / F``.  fp64 throughout, the dot products on the fp64 matrix cores; the Gram matrix is never written.  The order of the sums
    depends on (M, N, F) alone: two calls give the same bits, and the self form is symmetric bit for bit.  M, N >= 1, F a multiple
    of 16, ``KID_MIN_F`` <= F <= ``KID_MAX_F``.  ``out``: a contiguous fp64 device tensor [A,B] to write.  No host synchronisation."""
    M, F = _kid_features(x, 'x')
    N = M
    if y is not None:
        N, Fy = _kid_features(y, 'y')
        if Fy != F or y.device != x.device:
            raise ValueError('kid_tilesums_f64: y %s on %s does not match x %s on %s' % (tuple(y.shape), y.device, tuple(x.shape), x.device))
        if skip_diagonal:
            raise ValueError('kid_tilesums_f64: skip_diagonal is for the self form (y = None)')
    if M < 1 or N < 1 or F % 16 or not KID_MIN_F <= F <= KID_MAX_F:
        raise ValueError('kid_tilesums_f64: features [%d,%d] against [%d,%d] (at least one row a side, F a multiple of 16, %d <= F <= %d)'
                         % (M, F, N, F, KID_MIN_F, KID_MAX_F))
    gamma = 1.0 / F if gamma is None else float(gamma)
    A, B = (M + KID_TILE - 1) // KID_TILE, (N + KID_TILE - 1) // KID_TILE
    require_gpu()
    if out is None:
        out = torch.empty((A, B), device=x.device, dtype=torch.float64)
    else:
        _dev_tensor(out, torch.float64, (A, B), x.device, 'kid_tilesums_f64: out')
    _lib.call('pg_kid_tilesums_f64', x.data_ptr(), M, None if y is None else y.data_ptr(), N, F, gamma, float(coef0),
              1 if skip_diagonal else 0, out.data_ptr(), _stream())
    return out


# ------------------------------------------------------------------------- nearest windows at every start column (csrc/shift_search.hip)
SHIFT = {name[len('PG_SHIFT_'):]: value for name, value in _lib.SHIFT_CONSTANTS.items() if name.startswith('PG_SHIFT_')}   # the addition's own table
SHIFT_POS_BITS, SHIFT_MAX_QUERIES, SHIFT_TILE = SHIFT['POS_BITS'], SHIFT['MAX_QUERIES'], SHIFT['TILE']
SHIFT_MAX_SEG = 1 << SHIFT_POS_BITS                            # a key holds the start relative to its segment in POS_BITS bits
SHIFT_MIN_S, SHIFT_MAX_S = 4, 1024


def _shift_seg(S, seg):
    S = int(S)
    if S < SHIFT_MIN_S or S > SHIFT_MAX_S or S & (S - 1):
        raise ValueError('windows of %d rows (a power of two in %d .. %d is required)' % (S, SHIFT_MIN_S, SHIFT_MAX_S))
    if seg is None:
        seg = S
    if isinstance(seg, bool) or int(seg) != seg or not 1 <= seg <= SHIFT_MAX_SEG:
        raise ValueError('seg = %r (1 <= seg <= %d starts per segment)' % (seg, SHIFT_MAX_SEG))
    return S, int(seg)


def shift_segments(cols, S, seg=None):
    """The segment table of strips with ``cols`` columns searched with S x S windows: the starts 0 .. T_m - S of strip m are cut into
    segments of ``seg`` consecutive starts (default S), numbered strip-major.  Returns numpy int64 arrays ``(strip [G], first_start
    [G], first_segment [M + 1])``: the strip and the first start of every segment, and the first segment of every strip
    (``first_segment[M]`` = G).  Host arithmetic only."""
    import numpy as np
    S, seg = _shift_seg(S, seg)
    cols = [int(c) for c in cols]
    if not cols:
        raise ValueError('shift_segments: no strips')
    strip, start, first = [], [], [0]
    for m, T in enumerate(cols):
        if T < S:
            raise ValueError('strip %d: %d columns, a window needs %d' % (m, T, S))
        n = -(-(T - S + 1) // seg)
        strip.append(np.full(n, m, dtype=np.int64))
        start.append(np.arange(n, dtype=np.int64) * seg)
        first.append(first[-1] + n)
    return np.concatenate(strip), np.concatenate(start), np.asarray(first, dtype=np.int64)


def _shift_level(level, what):
    buf, table = level.buffer, level.table
    if not torch.is_tensor(buf) or not buf.is_cuda or buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.dim() != 1:
        raise ValueError('%s: level.buffer: expected a contiguous flat uint8 device tensor' % what)
    if (not torch.is_tensor(table) or table.device != buf.device or table.dtype != torch.int64 or not table.is_contiguous()
            or table.dim() != 2 or table.shape[0] != len(level.cols) or table.shape[0] < 1 or table.shape[1] != CROP_TABLE_WORDS):
        raise ValueError('%s: level.table: expected a contiguous int64 tensor [%d,%d] on the device of the buffer'
                         % (what, len(level.cols), CROP_TABLE_WORDS))


def shift_table(level, seg=None):
    """The int64 device table [M + 1, 2] that ``shift_l2min_u8`` hands to pg_shift_l2min_u8 for a ``dataset.StripLevel`` and a segment
    length: (first segment, first tile of ``SHIFT_TILE`` starts) of every strip, row M = (G, tiles).  Built on the host from
    ``level.cols`` and kept on the level: once per (level, seg)."""
    _shift_level(level, 'shift_table')
    S, seg = _shift_seg(level.S, seg)
    cache = level.__dict__.setdefault('_shift_tables', {})
    if seg not in cache:
        first = shift_segments(level.cols, S, seg)[2].tolist()
        tiles = [0]
        for T in level.cols:
            tiles.append(tiles[-1] + -(-(T - S + 1) // SHIFT_TILE))
        cache[seg] = torch.tensor(list(zip(first, tiles)), dtype=torch.int64).to(level.buffer.device)
    return cache[seg]


def shift_l2min_u8(level, queries_u8, seg=None, table=None):
    """One stored level of uint8 device strips (``dataset.StripLevel``, C channels, S rows) against uint8 device queries [K,C,S,S] ->
    int64 keys [K,G] (pg_shift_l2min_u8, on the int8 MFMA for S >= 32):

        key[k, g] = min over the starts u of segment g of  (d[k, m, u] << SHIFT_POS_BITS) + (u - first start of g),
        d[k, m, u] = sum_{c,r,j} (strip_m[c, r, u + j] - q_k[c, r, j])^2          (exact)

    with the segments of ``shift_segments(level.cols, S, seg)``: the minimum by (distance, start) over EVERY start column of the
    segment, so ``key >> SHIFT_POS_BITS`` is the squared distance and ``key & (SHIFT_MAX_SEG - 1)`` the start within the segment.
    The per-start distances are never stored: the only result is [K,G].  Every pass reads the level once for up to
    ``SHIFT_MAX_QUERIES`` queries; more take several passes, each into its own rows.  ``table``: the device table of
    ``shift_table(level, seg)`` if the caller keeps it.  No host synchronisation."""
    _shift_level(level, 'shift_l2min_u8')
    _u8_images(queries_u8, 'shift_l2min_u8 queries')
    S, seg = _shift_seg(level.S, seg)
    C, M = int(level.C), len(level.cols)
    if queries_u8.device != level.buffer.device or tuple(queries_u8.shape[1:]) != (C, S, S):
        raise ValueError('shift_l2min_u8: queries %s on %s do not match windows [%d,%d,%d] of the level on %s'
                         % (tuple(queries_u8.shape), queries_u8.device, C, S, S, level.buffer.device))
    if table is None:
        table = shift_table(level, seg)
    else:
        _dev_tensor(table, torch.int64, (M + 1, SHIFT['SEGTAB_WORDS']), level.buffer.device, 'shift_l2min_u8: table (of shift_table)')
    tiles = sum(-(-(T - S + 1) // SHIFT_TILE) for T in level.cols)
    G = sum(-(-(T - S + 1) // seg) for T in level.cols)
    K = queries_u8.shape[0]
    require_gpu()
    key = torch.empty((K, G), device=level.buffer.device, dtype=torch.int64)
    s = _stream()
    for k0 in range(0, K, SHIFT_MAX_QUERIES):
        k1 = min(K, k0 + SHIFT_MAX_QUERIES)
        _lib.call('pg_shift_l2min_u8', level.buffer.data_ptr(), level.table.data_ptr(), M, C, S, queries_u8[k0:k1].data_ptr(), k1 - k0, seg,
                  table.data_ptr(), tiles, G, key[k0:k1].data_ptr(), s)
    return key


# ------------------------------------------------------------------------- Griffin-Lim on the device (csrc/griffinlim.hip)
GL_MIN_N, GL_MAX_N = 8, 2048       # n_fft = 2 H: a power of two in this range (image heights 4 .. 1024)


def _f64_dev(t, what, ndim=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
        raise ValueError('%s: expected a contiguous float64 device tensor' % what)
    if ndim is not None and t.dim() != ndim:
        raise ValueError('%s: expected %d dimensions, got shape %s' % (what, ndim, tuple(t.shape)))
    return t


def _gl_n_fft(n_fft, what):
    if n_fft < GL_MIN_N or n_fft > GL_MAX_N or n_fft & (n_fft - 1):
        raise ValueError('%s: n_fft must be a power of two in %d .. %d, got %d' % (what, GL_MIN_N, GL_MAX_N, n_fft))


def gl_spectrum(images, mode='abslog', drange=(-1, 1)):
    """fp32 device images [n,H,W] (or [n,1,H,W]) -> the float64 spectrum [n, W frames, H + 1 bins] Griffin-Lim keeps
    (pg_gl_spectrum_f64, output_postprocess.py:109-118): zero-padded to H + 1 bins, THEN range-adjusted from ``drange`` to (0, 255)
    ('abslog': the value is the magnitude) or to (-1, 1) followed by (exp(|v|) - 1) * sign(v) ('reallog')."""
    if mode not in SOUND_MODES:
        raise ValueError("gl_spectrum: mode must be 'abslog' or 'reallog' (got %r)" % (mode,))
    _f32_dev(images, 'gl_spectrum images')
    if images.dim() == 4 and images.shape[1] == 1:
        images = images[:, 0]
    if images.dim() != 3 or images.shape[0] < 1:
        raise ValueError('gl_spectrum images: expected [n,H,W] or [n,1,H,W], got shape %s' % (tuple(images.shape),))
    n, H, W = images.shape
    _gl_n_fft(2 * H, 'gl_spectrum images of height %d' % H)
    range_out = (0, 255) if mode == 'abslog' else (-1, 1)
    lo_in, scale, lo_out = 0.0, 1.0, 0.0                     # adjust_dynamic_range (utils.py:24-30) leaves equal ranges untouched
    if tuple(drange) != range_out:
        lo_in, scale, lo_out = drange[0], (range_out[1] - range_out[0]) / (drange[1] - drange[0]), range_out[0]
    spec = torch.empty((n, W, H + 1), device=images.device, dtype=torch.float64)
    _lib.call('pg_gl_spectrum_f64', _p(images), spec.data_ptr(), n, H, W, float(lo_in), float(scale), float(lo_out),
              SOUND_MODES[mode], _stream())
    return spec


def _gl_shapes(spec, hop, what):
    _f64_dev(spec, what + ' spec', 3)
    batch, frames, bins = spec.shape
    hop = int(hop)
    n_fft = 2 * (bins - 1)
    _gl_n_fft(n_fft, what)
    if hop < 1 or batch < 1:
        raise ValueError('%s: hop must be >= 1 and the batch non-empty' % what)
    nsamp = hop * (frames - 1)
    if nsamp <= n_fft // 2:
        raise ValueError('%s: %d frames every %d samples give %d samples, reflect padding by n_fft/2 = %d needs more'
                         % (what, frames, hop, nsamp, n_fft // 2))
    return batch, frames, n_fft, hop, nsamp


def gl_pieces(x, spec, hop, out=None):
    """One Griffin-Lim round up to the overlap-add (pg_gl_pieces_f64): float64 device ``x`` [batch, hop (frames - 1)] and ``spec``
    [batch, frames, n_fft/2 + 1] -> windowed frames [batch, frames, n_fft] that carry spec's magnitudes and the phases of STFT(x).
    ``x`` None: the inverse transform of ``spec`` taken as a real spectrum ('reallog')."""
    batch, frames, n_fft, hop, nsamp = _gl_shapes(spec, hop, 'gl_pieces')
    if x is not None and tuple(_f64_dev(x, 'gl_pieces x', 2).shape) != (batch, nsamp):
        raise ValueError('gl_pieces x: expected [%d,%d], got %s' % (batch, nsamp, tuple(x.shape)))
    if out is None:
        out = torch.empty((batch, frames, n_fft), device=spec.device, dtype=torch.float64)
    elif tuple(_f64_dev(out, 'gl_pieces out', 3).shape) != (batch, frames, n_fft):
        raise ValueError('gl_pieces out: expected [%d,%d,%d], got %s' % (batch, frames, n_fft, tuple(out.shape)))
    _lib.call('pg_gl_pieces_f64', None if x is None else x.data_ptr(), nsamp, spec.data_ptr(), out.data_ptr(), n_fft, hop, frames,
              batch, _stream())
    return out


def overlap_add(pieces, hop, out=None):
    """float64 device frames [batch, frames, n_fft] -> signal [batch, hop (frames - 1)] (pg_overlap_add_f64): librosa's istft
    overlap-add with the centring pad cut off, the frames added in ascending order."""
    _f64_dev(pieces, 'overlap_add pieces', 3)
    batch, frames, n_fft = pieces.shape
    hop = int(hop)
    _gl_n_fft(n_fft, 'overlap_add')
    if hop < 1 or batch < 1 or frames < 2:
        raise ValueError('overlap_add: hop must be >= 1, the batch non-empty and frames >= 2')
    nsamp = hop * (frames - 1)
    if out is None:
        out = torch.empty((batch, nsamp), device=pieces.device, dtype=torch.float64)
    elif tuple(_f64_dev(out, 'overlap_add out', 2).shape) != (batch, nsamp):
        raise ValueError('overlap_add out: expected [%d,%d], got %s' % (batch, nsamp, tuple(out.shape)))
    _lib.call('pg_overlap_add_f64', pieces.data_ptr(), out.data_ptr(), nsamp, n_fft, hop, frames, batch, _stream())
    return out


def wave_normalize(x, repeat=1):
    """float64 device signals [batch, nsamp] -> float32 [batch, nsamp * repeat]: each divided by its peak max|x| in fp64, rounded to
    float32, every sample repeated ``repeat`` times (pg_wave_normalize_f32; output_postprocess.py:126, :152 and the WAV writer's cast)."""
    _f64_dev(x, 'wave_normalize x', 2)
    batch, nsamp = x.shape
    repeat = int(repeat)
    if batch < 1 or nsamp < 1 or repeat < 1:
        raise ValueError('wave_normalize: expected a non-empty [batch, nsamp] and repeat >= 1, got %s and %d' % (tuple(x.shape), repeat))
    peak = torch.empty(batch, device=x.device, dtype=torch.float64)
    out = torch.empty((batch, nsamp * repeat), device=x.device, dtype=torch.float32)
    _lib.call('pg_wave_normalize_f32', x.data_ptr(), _p(out), nsamp, repeat, batch, peak.data_ptr(), _stream())
    return out


def griffin_lim(images, x0, hop, rounds, mode='abslog', drange=(-1, 1), round_hook=None):
    """SoundSaver.image_to_sound up to the normalisation (output_postprocess.py:107-119) for a batch: fp32 device ``images`` [n,H,W]
    (or [n,1,H,W]) -> float64 device signals [n, hop (W - 1)].  'abslog': ``rounds`` rounds of Griffin-Lim from the float64 device
    starts ``x0`` [n, hop (W - 1)] (left unchanged); 'reallog': one inverse STFT (``x0`` and ``rounds`` unused).  1 + 2 rounds launches
    on the current stream (3 for 'reallog'), no host synchronisation -- unless ``round_hook(i, previous, x)`` is given, a debugging
    aid that is called with the two device signals after every round."""
    spec = gl_spectrum(images, mode, drange)
    if mode == 'reallog':
        return overlap_add(gl_pieces(None, spec, hop), hop)
    if x0 is None:
        raise ValueError("griffin_lim x0: 'abslog' needs the start signals")
    x = x0
    pieces = nxt = None
    for i in range(int(rounds)):
        pieces = gl_pieces(x, spec, hop, out=pieces)
        prev, x = x, overlap_add(pieces, hop, out=nxt)
        nxt = prev if prev is not x0 else None              # two signal buffers alternate; the caller's start is never written
        if round_hook is not None:
            round_hook(i, prev, x)
    return x


# ------------------------------------------------------------------------- loss and weight statistics (csrc/telemetry.hip)
STATS_MAX_SOURCES, STATS_RECORD = _C['PG_STATS_MAX_SOURCES'], _C['PG_STATS_RECORD']
STATS_MAX_LENGTH, SEG_CHUNK = _C['PG_STATS_MAX_LENGTH'], _C['PG_SEG_CHUNK']


def scalar_stats_record(K, device):
    """A record of ``K`` slots for ``scalar_stats_push``: float64 [K, STATS_RECORD] on ``device``, uninitialised (the first push
    carries ``reset=True``)."""
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= STATS_MAX_SOURCES:
        raise ValueError('scalar_stats_record: %r slots (1 .. %d)' % (K, STATS_MAX_SOURCES))
    return torch.empty((int(K), STATS_RECORD), device=device, dtype=torch.float64)


def scalar_stats_push(record, sources, reset=False):
    """Fold the means of up to ``STATS_MAX_SOURCES`` small fp32 device tensors into ``record`` (``scalar_stats_record``), slot k from
    ``sources[k]`` (None: the slot is skipped): ONE launch on the current stream, no copy, no host synchronisation
    (pg_scalar_stats_push; the record's layout and the order of the sums are stated in include/pggan_hip.h).  ``reset``: every slot is
    put into its empty state before the sources are folded.  A source is contiguous with 1 .. ``STATS_MAX_LENGTH`` elements of any shape."""
    if (not torch.is_tensor(record) or not record.is_cuda or record.dtype != torch.float64 or not record.is_contiguous()
            or record.dim() != 2 or record.shape[1] != STATS_RECORD or not 1 <= record.shape[0] <= STATS_MAX_SOURCES):
        raise ValueError('scalar_stats_push: record must be a contiguous float64 device tensor [K <= %d, %d]' % (STATS_MAX_SOURCES, STATS_RECORD))
    K = record.shape[0]
    if len(sources) != K:
        raise ValueError('scalar_stats_push: %d sources for a record of %d slots' % (len(sources), K))
    ptrs, lens = (ctypes.c_void_p * K)(), (ctypes.c_int * K)()
    for k, t in enumerate(sources):
        if t is None:
            continue
        if (not torch.is_tensor(t) or t.device != record.device or t.dtype != torch.float32 or not t.is_contiguous()
                or not 1 <= t.numel() <= STATS_MAX_LENGTH):
            raise ValueError('scalar_stats_push: source %d must be a contiguous float32 tensor of 1 .. %d elements on %s'
                             % (k, STATS_MAX_LENGTH, record.device))
        ptrs[k], lens[k] = t.data_ptr(), t.numel()
    require_gpu()
    _lib.call('pg_scalar_stats_push', record.data_ptr(), ptrs, lens, K, 1 if reset else 0, _stream())
    return record


def segment_stats_plan(segments, n_flat):
    """The chunk table of ``segment_stats`` for ``segments`` = [(offset, length), ...] of a flat buffer of ``n_flat`` floats, cut by the
    library's own rule (pg_segment_stats_plan; host only, no device): ``(chunks [nchunks, 2], ranges [S, 2])`` int64 host tensors.
    An offset that is no multiple of 4 elements is PG_E_ALIGN, a segment outside the buffer or an empty one PG_E_ARG (RuntimeError)."""
    S = len(segments)
    if S < 1:
        raise ValueError('segment_stats_plan: no segments')
    offs = (ctypes.c_int64 * S)(*[int(o) for o, _ in segments])
    lens = (ctypes.c_int64 * S)(*[int(n) for _, n in segments])
    count = ctypes.c_int64(0)
    _lib.call('pg_segment_stats_plan', offs, lens, S, int(n_flat), None, 0, None, ctypes.addressof(count))
    chunks = torch.empty((count.value, 2), dtype=torch.int64)
    ranges = torch.empty((S, 2), dtype=torch.int64)
    _lib.call('pg_segment_stats_plan', offs, lens, S, int(n_flat), chunks.data_ptr(), count.value, ranges.data_ptr(), ctypes.addressof(count))
    return chunks, ranges


def segment_stats(flat, chunks, ranges, partials=None):
    """{sum, sumsq, maxabs, n_nonfinite} over the finite elements of every segment of the flat fp32 device buffer ``flat``: float64
    device tensor [S, 4] (pg_segment_stats_f32 + pg_segment_stats_finish: two launches on the current stream, no atomics, the same
    bits for the same input, a segment's numbers independent of the other segments').  ``chunks`` / ``ranges``: the tables of
    ``segment_stats_plan(segments, flat.numel())`` as int64 tensors ON THE DEVICE (uploaded once by the caller).  ``partials``: float64
    device scratch [nchunks, 4] to reuse."""
    if not torch.is_tensor(flat) or not flat.is_cuda or flat.dtype != torch.float32 or not flat.is_contiguous() or flat.numel() < 1:
        raise ValueError('segment_stats: expected a contiguous, non-empty float32 device tensor')
    for t, what in ((chunks, 'chunks'), (ranges, 'ranges')):
        if (not torch.is_tensor(t) or t.device != flat.device or t.dtype != torch.int64 or not t.is_contiguous() or t.dim() != 2
                or t.shape[1] != 2 or t.shape[0] < 1):
            raise ValueError('segment_stats: %s must be a contiguous int64 tensor [n, 2] on the device of the buffer' % what)
    nchunks, S = chunks.shape[0], ranges.shape[0]
    if partials is None:
        partials = torch.empty((nchunks, 4), device=flat.device, dtype=torch.float64)
    elif (not torch.is_tensor(partials) or partials.device != flat.device or partials.dtype != torch.float64
          or not partials.is_contiguous() or tuple(partials.shape) != (nchunks, 4)):
        raise ValueError('segment_stats: partials must be a contiguous float64 tensor [%d, 4] on the device of the buffer' % nchunks)
    require_gpu()
    out = torch.empty((S, 4), device=flat.device, dtype=torch.float64)
    s = _stream()
    _lib.call('pg_segment_stats_f32', flat.data_ptr(), flat.numel(), chunks.data_ptr(), nchunks, partials.data_ptr(), s)
    _lib.call('pg_segment_stats_finish', partials.data_ptr(), nchunks, ranges.data_ptr(), S, out.data_ptr(), s)
    return out


# ------------------------------------------------------------------------- pyramid loss of the latent projection (csrc/projection.hip)
PYR = {name[len('PG_PYR_'):]: value for name, value in _lib.PROJECTION_CONSTANTS.items() if name.startswith('PG_PYR_')}   # the addition's own table
PYR_TILE, PYR_MAX_SIDE, PYR_MAX_C, PYR_SCRATCH_PER_TILE = PYR['TILE'], PYR['MAX_SIDE'], PYR['MAX_C'], PYR['SCRATCH_PER_TILE']


def pyramid_levels(r):
    """Levels of the box-mean pyramid of an r x r image: sides r, r/2, .., 4."""
    return int(r).bit_length() - 2


def pyramid_scratch_words(N, C, r):
    """fp64 words of scratch ``pyramid_loss`` needs for a batch [N,C,r,r]."""
    return PYR_SCRATCH_PER_TILE * N * C * (r // min(r, PYR_TILE)) ** 2


def pyramid_loss(img, target, weights=None, want_grad=True, scratch=None):
    """Multi-resolution squared error of two fp32 device batches [N,C,r,r] (r a power of two in 4 .. 1024, C in 1 .. 4) and its gradient
    with respect to ``img`` (pg_pyr_loss_grad, include/pggan_hip_projection.h):

        loss[n] = sum_l w_l mean_{c,y,x} P_l(img - target)[n]^2,    P_l the l-fold 2x2 box mean, sides r .. 4

    ``weights``: a sequence of up to ``pyramid_levels(r)`` non-negative floats, w_l of the levels from the finest (missing ones are 0);
    None: every level 1.  Returns ``(loss [N], grad [N,C,r,r])``, fp32 device tensors; ``want_grad=False`` gives ``(loss, None)`` in one
    pass over the images.  fp64 sums in a fixed order, one rounding per output, no atomics: two calls give the same bits.  ``scratch``:
    a float64 device tensor of at least ``pyramid_scratch_words(N, C, r)`` elements to reuse.  No host synchronisation."""
    for t, name in ((img, 'img'), (target, 'target')):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('pyramid_loss %s: expected a contiguous float32 device tensor' % name)
    if img.dim() != 4 or img.shape != target.shape or img.device != target.device:
        raise ValueError('pyramid_loss: expected two equal shapes [N,C,r,r] on one device, got %s and %s' % (tuple(img.shape), tuple(target.shape)))
    N, C, r, W = img.shape
    if N < 1 or not 1 <= C <= PYR_MAX_C or r != W or r < 4 or (r & (r - 1)) or r > PYR_MAX_SIDE:
        raise ValueError('pyramid_loss: expected [N,C,r,r] with N >= 1, C in 1 .. %d and r a power of two in 4 .. %d, got %s'
                         % (PYR_MAX_C, PYR_MAX_SIDE, tuple(img.shape)))
    wbuf, nlev = None, 0
    if weights is not None:
        ws = [float(w) for w in weights]
        nlev = len(ws)
        if not 1 <= nlev <= pyramid_levels(r) or any(not (0.0 <= w < float('inf')) for w in ws):
            raise ValueError('pyramid_loss: weights must be 1 .. %d finite non-negative numbers for r = %d, got %r' % (pyramid_levels(r), r, ws))
        wbuf = (ctypes.c_float * nlev)(*ws)
    words = pyramid_scratch_words(N, C, r)
    if scratch is None:
        scratch = torch.empty(words, device=img.device, dtype=torch.float64)
    elif (not torch.is_tensor(scratch) or scratch.device != img.device or scratch.dtype != torch.float64 or not scratch.is_contiguous()
          or scratch.numel() < words):
        raise ValueError('pyramid_loss: scratch must be a contiguous float64 tensor of at least %d elements on the device of the images' % words)
    require_gpu()
    loss = torch.empty(N, device=img.device, dtype=torch.float32)
    grad = torch.empty_like(img) if want_grad else None
    _lib.call('pg_pyr_loss_grad', img.data_ptr(), target.data_ptr(), ctypes.cast(wbuf, ctypes.c_void_p) if wbuf is not None else None, nlev,
              grad.data_ptr() if grad is not None else None, loss.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, N, C, r, _stream())
    return loss, grad


# ------------------------------------------------------------------------- differentiable augmentation of D's inputs (csrc/augment.hip)
AUGMENT = {name[len('PG_AUGMENT_'):]: value for name, value in _lib.AUGMENT_CONSTANTS.items() if name.startswith('PG_AUGMENT_')}   # the addition's own table
AUGMENT_COLS, AUGMENT_FLIP, AUGMENT_GAIN = AUGMENT['COLS'], AUGMENT['FLIP'], AUGMENT['GAIN']
AUGMENT_MAX_SIZE, AUGMENT_MAX_SCORES = AUGMENT['MAX_SIZE'], AUGMENT['MAX_SCORES']


def _augment_table(table, n, what):
    if (not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.int32 or not table.is_contiguous()
            or tuple(table.shape) != (n, AUGMENT_COLS)):
        raise ValueError('%s: the table must be a contiguous int32 device tensor [%d, %d]' % (what, n, AUGMENT_COLS))
    return table.data_ptr()


def augment_apply(x, table, channel_mask=0, out=None):
    """``out[n]`` = image ``x[n]`` [C,H,W] flipped, shifted with zero padding, cut out and (channels of ``channel_mask``) raised by the
    gain, as row ``n`` of the int32 ``table`` [N,8] says (pg_augment_apply; include/pggan_hip_augment.h has the definition).  One launch
    on the current stream, every element of ``out`` written."""
    y = out if out is not None else torch.empty_like(x)
    N, C, H, W = x.shape
    _lib.call('pg_augment_apply', _p(x), _augment_table(table, N, 'augment_apply'), _p(y), N, C, H, W, int(channel_mask), _stream())
    return y


def augment_adjoint(gy, table, out=None):
    """The exact transpose of ``augment_apply`` under the same ``table``: ``gx[p] = gy[q]`` for the one output pixel q whose source is p,
    +0.0 where there is none or q lies in the cutout (pg_augment_adjoint)."""
    gx = out if out is not None else torch.empty_like(gy)
    N, C, H, W = gy.shape
    _lib.call('pg_augment_adjoint', _p(gy), _augment_table(table, N, 'augment_adjoint'), _p(gx), N, C, H, W, _stream())
    return gx


def augment_table(U, H, W, ry, rx, ch, cw, gain, flip, p, out=None):
    """U[0,1) draws ``U`` [rows,8] (``uniform_``) -> the int32 parameter table [rows,8] of a policy at probability ``p`` (pg_augment_table)."""
    if not torch.is_tensor(U) or not U.is_cuda or U.dtype != torch.float32 or not U.is_contiguous() or U.dim() != 2 or U.shape[1] != AUGMENT_COLS:
        raise ValueError('augment_table: expected a contiguous float32 device tensor [rows, %d]' % AUGMENT_COLS)
    rows = U.shape[0]
    table = out if out is not None else torch.empty((rows, AUGMENT_COLS), device=U.device, dtype=torch.int32)
    _lib.call('pg_augment_table', _p(U), rows, H, W, ry, rx, ch, cw, gain, int(bool(flip)), p, _augment_table(table, rows, 'augment_table'),
              _stream())
    return table


def score_signs(scores, acc):
    """``acc[0] += sum sign(scores)`` (sign(+-0) = 0), ``acc[1] += scores.numel()`` on the fp64 device accumulator ``acc`` [2]
    (pg_score_signs: one workgroup, exact)."""
    if not torch.is_tensor(acc) or not acc.is_cuda or acc.dtype != torch.float64 or not acc.is_contiguous() or acc.numel() != 2:
        raise ValueError('score_signs: the accumulator must be a contiguous float64 device tensor of 2 elements')
    _lib.call('pg_score_signs', _p(scores), scores.numel(), acc.data_ptr(), _stream())
    return acc
