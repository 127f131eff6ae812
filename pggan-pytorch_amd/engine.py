"""Explicit launch schedules of the PGGAN hot path (no autograd graph, no tracing compiler).

Every pass below is a hand-ordered sequence of the C-ABI kernels (``ops``):

  generator_forward / generator_backward            reference network.py:118-139 + its autograd
  discriminator forward (batched [real|fake|mixed])  reference network.py:225-240
  d_backward            first-order adjoint sweep (data-only or data+weights): the driver of
                        _consume | _pn_adjoints (seed: _pn_head_seed) -> _hand_over (+ _fade_in) ... -> _entry, which pass saved.PoolAdjoint between blocks
  _bytes_first          the one rule for LeakyReLU' masks kept as sign bytes (saved.Sign): bytes first, fp32 when a launch refuses
  d_tangent_wgrad       forward-mode (tangent) sweep of the gradient-penalty second-order term

The WGAN-GP double backward (wgan_gp_loss.py:25-31 + trainer.py:98) is NOT done with a generic
autograd.  With default flags D is piecewise linear except for minibatch-stddev, so

    d/dtheta  sum_i gp_i / N   =   d/dtheta  < u , grad_x S(x^, theta) >        (u held constant)
                               =   grad_theta of the directional derivative of S along u

which is evaluated as (i) a tangent pass pushing u through the same masked linear maps,
(ii) weight gradients  tangent_input (x) first-backward-adjoint  per layer, and (iii) the
minibatch-stddev Hessian-vector term injected into the ordinary batched backward of the mixed
samples (SURVEY.md §7 "hard parts"; formulas verified against autograd in tests/).
"""
import collections as _collections
import contextlib as _contextlib
import os
import weakref as _weakref

import torch

from . import ops
from . import saved


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def _check_dev(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError('%s must be a tensor on the MI355X device (no CPU path exists); got %s'
                           % (what, getattr(t, 'device', type(t))))
    if t.dtype != torch.float32:
        raise RuntimeError('%s must be float32' % what)
    return t.contiguous()


# Winograd F(2x2,3x3) (csrc/conv_wino.hip) replaces the direct implicit GEMM where it measured faster (tools/sweeps/sweep_wino.py):
# 3x3 layers with a full 16-cout MFMA tile and enough 64-tile workgroups to fill the chip.  With the second-generation kernel
# (8-channel chunks) that includes the 16-channel layers of the 512^2 stage (1.3-1.55x the direct kernel) and 8->16 at 1024^2
# (1.16x); 16->8 and 8->8 (half of the cout tile empty) stay on the block-MFMA kernels (0.7-1.0x).
USE_WINOGRAD = True            # False in tests/test_winograd.py::test_engine_with_sign_bytes_gpu: every 3x3 layer on the direct kernels
WINO_MIN_WORKGROUPS = 32       # (K is sliced across workgroups below ~432: ops._stream_with_workspace); 0 in tests/test_winograd.py::_engine_vs_oracle
_WINO_MIN_CHANNELS = 8         # input channels of the conv
_WINO_MIN_COUT = 16            # a full 16-cout MFMA tile
_WINO_WGRAD_MIN_CHANNELS = 16  # channels (either side) of a Winograd weight gradient
# The c2 output of a DBlock is pooled at once (network.py:229,238); at full resolution only its SIGN is ever used again
# (LeakyReLU' in the backward / tangent sweeps), so from 64x64 up it is kept as sign bytes (1 byte per 4 channels)
# instead of fp32: the fp32 write and its re-reads are the largest avoidable HBM traffic of the high-resolution stages.
FALLBACKS = _collections.Counter()       # launches that answered PG_E_UNSUP to a sign-byte request and were redone in fp32
USE_SIGN_BYTES = True          # tests/test_winograd.py::test_engine_with_sign_bytes_host / _gpu set both (sign bytes from 8x8 up)
SIGN_BYTES_MIN_H = 64
# With the mask as sign bytes the pool adjoint between two DBlocks can be evaluated in the input gathers of its consumers
# (backward-data conv and weight gradient of the finer block's c2) instead of being written out at the fine resolution.
USE_LAZY_UNPOOL = True         # tests/test_winograd.py::test_engine_with_lazy_pool_adjoint_gpu checks that the path is taken


def _live_conv_layers(net):
    """3x3 / 4x4 conv layers that can run at the network's current growth stage (D: blocks[-(depth+1):], network.py:227-238;
    G: ``Generator.stage_convs``)."""
    depth = int(net.depth)
    if not hasattr(net, 'linear'):                              # Generator
        return [lay for _, lay in net.stage_convs(depth)]
    blocks = list(net.blocks)[len(net.blocks) - 1 - depth:]
    return [m for b in blocks for m in (b.c1, b.c2)]


def _derived(net):
    """Derived weight copies of a network, refreshed with three launches per (weight version, growth stage): backward-data
    (flipped / transposed) weights, and the Winograd-domain forward and backward-data weights — of the layers that are live
    at this stage only (at 4x4 that is 2 of the 18 conv layers of a network: re-deriving all 73 MB per update cost ~0.5 ms of
    a 1.6 ms step)."""
    net._ensure_buffers()
    rt = net._rt
    key = (net._param_version, int(net.depth))
    if rt.derived_ver == key:
        return
    base = net._flat_param.data_ptr()
    live = set(id(m) for m in _live_conv_layers(net))
    # flipped / transposed copies: only for the layers whose backward-data conv has asked for one (_wt marks them) -- the layers that
    # always run Winograd there get their backward-data form straight from the parameter (transposed=True below)
    todo = [m for m in net._layers() if m.kind == 'conv' and m._wt is not None and id(m) in live and m._wt_wanted]
    packs = [((m.conv.weight.data_ptr() - base) // 4, m.ksize, m.conv.weight.shape[2], m.conv.weight.shape[3]) for m in todo]
    # ... and of those only the layers the Winograd path has actually asked for (_wino marks them): the 512-channel layers of the
    # 4x4 stage never reach it, yet are a large part of all Winograd-domain bytes
    wl = [(m, woff, uoff) for m, woff, uoff in (net._wino_layers or []) if id(m) in live and m._wino_wanted]
    wl = wl if USE_WINOGRAD else []

    def backward_copies():                       # what only the backward-data convs read: flipped / transposed weights and the Winograd form of those
        if packs:
            ops.pack_dgrad_weights_batched(net._flat_param, net._flat_wt, packs)
        if wl:
            ops.wino_transform_weights_batched(net._flat_param, net._flat_wtu,
                                               [(woff, uoff, m.conv.weight.shape[3], m.conv.weight.shape[2]) for m, woff, uoff in wl],
                                               transposed=True)
    dev = torch.cuda.current_device() if net._flat_param.is_cuda else None
    cur = torch.cuda.current_stream(torch._C._cuda_getDevice()) if dev is not None else None
    capturing = dev is not None and torch.cuda.is_current_stream_capturing()
    # Inside a deferred update (defer_to_side: Adam + this refresh on the second stream while the main stream waits for D's weights -- since
    # round 6's early generator pass that wait is exposed, tools/phase_timeline.py) the forward forms go first and close the update for
    # the waiting stream (``_rt.pending`` = the event behind them); the backward-data forms and the flipped copies follow behind that event and
    # are picked up through ``_await_backward_copies`` by their first reader, a forward pass later.
    split = rt.defer_active and dev is not None and cur == _SIDE.get(dev) and not capturing
    one_launch = bool(wl) and rt.bwd_wanted and not split
    if one_launch:
        # forward AND backward-data Winograd forms in one launch on this stream (the two forms share a buffer, network._flat_wuu): the
        # parameter is read while it is hot, no second launch, no cross-stream hop for it at the iteration boundary
        half = net._flat_wu.numel()
        ops.wino_transform_weights_batched(
            net._flat_param, net._flat_wuu,
            [(woff, uoff, m.conv.weight.shape[2], m.conv.weight.shape[3]) for m, woff, uoff in wl] +
            [(woff, half + uoff, m.conv.weight.shape[3], m.conv.weight.shape[2]) for m, woff, uoff in wl],
            transposed=[False] * len(wl) + [True] * len(wl))
        wl = []                                  # (backward_copies below: only the flipped copies of the direct-conv layers are left)
    elif wl:                                     # the forward convs' Winograd-domain weights: needed by the very next launch
        ops.wino_transform_weights_batched(net._flat_param, net._flat_wu,
                                           [(woff, uoff, m.conv.weight.shape[2], m.conv.weight.shape[3]) for m, woff, uoff in wl])
    # The backward copies are not needed before the network's next backward sweep (milliseconds away): off the critical path, onto
    # the weight-gradient stream, unless this already IS that stream (the deferred D update) or a hipGraph is being captured.
    # A network that has never run a backward sweep (an EMA / evaluation copy) gets none: the first request for one
    # (_wt / _wino(transposed)) invalidates the derived state.
    # The forward forms are on ``cur`` now.  A consumer on ANOTHER stream must be ordered behind them (_await_derived): the three-pass D
    # forward refreshes D's derived weights from inside its real-third pass on the second stream whenever the update did not come through
    # Trainer's deferred update -- the public ``loss.backward(); optimizer.step()`` loop, a foreign optimizer, load_state_dict -- while the
    # mixed third on the main stream was ordered behind the image copy only (docs/experiments_r6.md §1).
    rt.derived_ev = None
    rt.derived_waited = set()
    if dev is not None and DERIVED_EVENT and not capturing:
        ev = torch.cuda.Event()
        _record_event(ev, cur)
        rt.derived_ev = ev
        rt.derived_waited = {cur.cuda_stream}
        if split:
            rt.pending_ev = ev
    rt.derived_bwd_ev = None
    rt.derived_bwd_waited = set()
    if not rt.bwd_wanted:
        pass
    elif ASYNC_WGRAD and dev is not None and cur != _SIDE.get(dev) and not capturing:
        side = _side_stream()
        _wait_stream(side, cur)
        with torch.cuda.stream(side):
            backward_copies()
            ev = torch.cuda.Event()
            _record_event(ev, side)
        for buf in (net._flat_wt, net._flat_wtu):  # written on the side stream: the allocator must not hand the block on before that
            if buf is not None:
                buf.record_stream(side)
        rt.derived_bwd_ev = ev
    else:
        backward_copies()                        # inline, on ``cur``: readers on other streams are ordered behind this event
        if dev is not None and DERIVED_EVENT and not capturing:
            ev = torch.cuda.Event()
            _record_event(ev, cur)
            rt.derived_bwd_ev = ev
            rt.derived_bwd_waited = {cur.cuda_stream}
    rt.derived_ver = key
    rt.derived_live = live


def _await_derived(net):
    """The current stream waits (once) for the last refresh of the derived weights if that ran on another stream."""
    ev = net._rt.derived_ev
    if ev is not None:
        cur = torch.cuda.current_stream(torch._C._cuda_getDevice())
        waited = net._rt.derived_waited
        if cur.cuda_stream not in waited and not torch.cuda.is_current_stream_capturing():
            cur.wait_event(ev)
            waited.add(cur.cuda_stream)


def order_side_behind_derived(net):
    """plans.py, before a replay: the recorded body's per-launch ``_await_derived`` calls are not part of a plan (they are no-ops in
    the orders a plan is entered with), so the one ordering a replay could miss -- the second stream behind a refresh ``_prologue`` just
    issued on the main stream -- is established here, once per step."""
    ev = net._rt.derived_ev
    if ev is not None and ASYNC_WGRAD:
        side = _side_stream()
        if side.cuda_stream not in net._rt.derived_waited:
            side.wait_event(ev)
            net._rt.derived_waited.add(side.cuda_stream)


def _assert_live(net, layer):
    """The derived copies are refreshed for the layers that are live at the network's current growth stage only: asking for
    any other layer's would silently compute with the weights of an earlier optimizer step."""
    if id(layer) not in net._rt.derived_live:
        raise RuntimeError('derived weights requested for a conv layer that is not live at depth %d' % int(net.depth))


def _await_backward_copies(net):
    """The current stream waits for the side-stream refresh of the backward-only derived weights.  The event stays until the
    next refresh, so that EVERY stream that consumes (or, for the optimizer, overwrites the source of) the copies is ordered
    behind it, each once."""
    ev = net._rt.derived_bwd_ev
    if ev is not None:
        cur = torch.cuda.current_stream(torch._C._cuda_getDevice())
        waited = net._rt.derived_bwd_waited
        if cur.cuda_stream not in waited:
            _wait_event(cur, ev)
            waited.add(cur.cuda_stream)


def _want_backward_copies(net):
    if not net._rt.bwd_wanted:                          # first backward sweep of this network: from now on every refresh includes them
        net._rt.bwd_wanted = True
        net._rt.derived_ver = None


def _wt(net, layer):
    """Backward-data (flipped/transposed) copy of a conv layer's weights, refreshed lazily."""
    if not layer._wt_wanted:                            # first request: from now on the refresh after every update includes this layer
        layer._wt_wanted = True
        net._rt.derived_ver = None
    _want_backward_copies(net)
    _derived(net)
    _assert_live(net, layer)
    _await_derived(net)
    _await_backward_copies(net)
    return layer._wt


def _wino(layer, N, H, cout, transposed=False):
    """Winograd-domain weights of ``layer`` if that path should run for an N x H x H output with ``cout`` channels."""
    if not USE_WINOGRAD or getattr(layer, '_wu', None) is None or H < 8:
        return None
    cin = layer.conv.weight.shape[2] if transposed else layer.conv.weight.shape[3]     # input channels of THIS direction
    if cin < _WINO_MIN_CHANNELS or cout < _WINO_MIN_COUT:
        return None
    if -(-(N * (H // 2) * (H // 2)) // 64) * -(-cout // 16) < WINO_MIN_WORKGROUPS:
        return None
    net = layer._net()
    if not layer._wino_wanted:                          # first request: from now on the refresh after every update includes this layer
        layer._wino_wanted = True
        net._rt.derived_ver = None
    if transposed:
        _want_backward_copies(net)
    _derived(net)
    _assert_live(net, layer)
    _await_derived(net)
    if transposed:
        _await_backward_copies(net)
    return layer._wtu if transposed else layer._wu


def _f32(sign):
    """fp32 view of a LeakyReLU' mask that may be stored as sign bytes only (paths without a byte-aware kernel)."""
    return sign.f32 if sign.f32 is not None or sign.bytes is None else ops.signbytes_to_mask(sign.bytes)


def _bytes_first(run, sign, tag, bytes_out=False, count=True, redo=None):
    """THE rule for a launch that may be handed sign bytes.

    First attempt: ``run(mask, bytes_out)`` with the bytes of ``sign`` (a saved.Sign or None) as the mask.  ``bytes_out`` asks for a
    byte OUTPUT (signs_out / y_bytes) as well.
    If that answers ``ops.Unsupported``, the launch is counted under ``FALLBACKS[tag]`` and redone as ``run(fp32 mask, False)``.
    The fp32 copy is used as given; the bytes are expanded only when there is none.
    With no byte in play there is nothing to redo: ``Unsupported`` is the caller's.

    tag   : the key, or a callable that formats it (only a counted fallback pays for the string).
    count : False redoes silently.
    redo  : called in place of the second ``run``, by a launch that has to expand the bytes itself, behind what its other arguments
            issue."""
    mb = sign.bytes if sign is not None else None
    if mb is None and not bytes_out:
        return run(sign.f32 if sign is not None else None, False)
    try:
        return run(mb if mb is not None else sign.f32 if sign is not None else None, bytes_out)
    except ops.Unsupported:
        if count:
            FALLBACKS[tag() if callable(tag) else tag] += 1
    return redo() if redo is not None else run(None if sign is None else _f32(sign), False)


def _conv(x, layer, N, H, act=True, mask=None, bias=True, ups=False, out=None, signs_out=False):
    """Forward conv (+bias+act) or, with ``mask`` (the saved.Sign of the layer's own output), the masked linear map of the tangent
    pass.  ``signs_out``: returns (y, sign bytes of y) -- (y, None) when the launch cannot produce them."""
    def run(m, so):
        u = _wino(layer, N, H, layer.conv.weight.shape[2])
        if u is not None:
            y = ops.conv2d_wino(x, u, layer.conv.bias.data if bias else None, N, H, H, layer.c,
                                layer.slope if act else 1.0, mask=m, mask_slope=layer.slope, ups=ups, out=out, signs_out=so)
        else:
            y = ops.conv2d(x, layer.conv.weight.data, layer.conv.bias.data if bias else None, N, H, H,
                           layer.ksize, layer.pad, layer.c, layer.slope if act else 1.0,
                           mask=m, mask_slope=layer.slope, ups=ups, out=out, signs_out=so)
        return (y, None) if signs_out and not so else y
    if not signs_out and (mask is None or mask.bytes is None):         # (no byte in play: nothing for the rule, one call less on the host)
        return run(mask and mask.f32, False)
    return _bytes_first(run, mask, lambda: 'conv %s %dx%d %s' % ('signs_out' if signs_out else 'masked', H, H, tuple(layer.conv.weight.shape)),
                        bytes_out=signs_out)


def _conv_pool(x, layer, N, H, bias=True, mask=None, other=None, a=1.0, b=0.0, pool_only=False, y_bytes=False):
    """conv (+bias+act | mask: as in ``_conv``) followed by the 2x2 average pool / fade-in blend, one launch.  ``y_bytes``: the
    full-resolution output is returned as sign bytes (falls back to fp32 when the launch cannot fuse)."""
    def run(m, yb):
        u = _wino(layer, N, H, layer.conv.weight.shape[2])
        if u is not None:
            return ops.conv2d_wino(x, u, layer.conv.bias.data if bias else None, N, H, H, layer.c,
                                   layer.slope if m is None else 1.0, mask=m, mask_slope=layer.slope,
                                   pool=True, other=other, a=a, b=b, pool_only=pool_only, y_bytes=yb)
        return ops.conv2d_pool(x, layer.conv.weight.data, layer.conv.bias.data if bias else None, N, H, H, layer.ksize, layer.pad,
                               layer.c, layer.slope if m is None else 1.0, mask=m, mask_slope=layer.slope,
                               other=other, a=a, b=b, pool_only=pool_only, y_bytes=yb)
    if not y_bytes and (mask is None or mask.bytes is None):
        return run(mask and mask.f32, False)
    return _bytes_first(run, mask, lambda: 'conv_pool %dx%d %s' % (H, H, tuple(layer.conv.weight.shape)), bytes_out=y_bytes)


def _dgrad(net, gz, layer, N, Hout, mask=None):
    """Adjoint of the conv wrt its input: gz [N,Hout,Hout,Cout] -> [N,Hin,Hin,Cin_store] (* LeakyReLU' of ``mask``, a saved.Sign)."""
    slope = mask.slope if mask is not None else 0.2

    def run(m, _):
        u = _wino(layer, N, Hout, layer.conv.weight.shape[3], transposed=True) if layer.ksize == 3 and layer.pad == 1 else None
        if u is not None:
            return ops.conv2d_wino(gz, u, None, N, Hout, Hout, layer.c, 1.0, mask=m, mask_slope=slope)
        return ops.conv2d(gz, _wt(net, layer), None, N, Hout, Hout, layer.ksize, layer.ksize - 1 - layer.pad,
                          layer.c, 1.0, mask=m, mask_slope=slope)
    if mask is None or mask.bytes is None:
        return run(mask and mask.f32, False)
    return _bytes_first(run, mask, lambda: 'dgrad masked %dx%d %s' % (Hout, Hout, tuple(layer.conv.weight.shape)))


def _dgrad_pool(net, gz, layer, N, H, other=None, a=1.0, b=0.0, pnb=None):
    """Backward-data conv + 2x2 pooled epilogue (a * mean + b * other); only the pooled result is produced.
    ``pnb`` = (ysaved, r, slope): the adjoint of the coarser block's last (LeakyReLU -> PixelNorm) follows -- in the same launch
    where the Winograd epilogue holds every channel of the pooled pixel.  Returns (result, adjoint applied?)."""
    u = _wino(layer, N, H, layer.conv.weight.shape[3], transposed=True)
    if pnb is not None:
        if u is not None and u.shape[1] <= 32 and pnb[1] is not None:
            return ops.conv2d_wino_pnbwd(gz, u, pnb[0], pnb[1], N, H, H, layer.c, pnb[2], pool=True, other=other, a=a, b=b), True
        return _dgrad_pool(net, gz, layer, N, H, other=other, a=a, b=b), False
    if u is not None:
        return ops.conv2d_wino(gz, u, None, N, H, H, layer.c, 1.0, pool=True, other=other, a=a, b=b, pool_only=True)[1]
    return ops.conv2d_pool(gz, _wt(net, layer), None, N, H, H, layer.ksize, layer.ksize - 1 - layer.pad, layer.c, 1.0,
                           other=other, a=a, b=b, pool_only=True)[1]


def _dgrad_unpool(net, gz, layer, N, H, up, mul):
    """Backward-data conv + pool adjoint + LeakyReLU' of the finer activation (``up``, a saved.Sign), one launch."""
    u = _wino(layer, N, H, layer.conv.weight.shape[3], transposed=True)
    if u is not None:                              # (outside the rule: this launch takes either form, a refusal is the caller's)
        return ops.conv2d_wino(gz, u, None, N, H, H, layer.c, 1.0, mask_slope=up.slope, unpool=True,
                               upmask=up.bytes if up.bytes is not None else up.f32, up_mul=mul)

    def launch(mask):                              # mask(): read behind the wait for the weights, where the redo expands the bytes
        return ops.conv2d_unpool(gz, _wt(net, layer), N, H, H, layer.ksize, layer.ksize - 1 - layer.pad, layer.c,
                                 upmask=mask(), mul=mul, mask_slope=up.slope)
    return _bytes_first(lambda m, _: launch(lambda: m), up, lambda: 'dgrad unpool %dx%d %s' % (H, H, tuple(layer.conv.weight.shape)),
                        redo=lambda: launch(lambda: _f32(up)))


def _dgrad_pnbwd(net, gz, layer, N, H, ysaved, r, slope):
    """Backward-data conv + adjoint of the previous layer's (LeakyReLU -> PixelNorm)."""
    u = _wino(layer, N, H, layer.conv.weight.shape[3], transposed=True)
    if u is not None and u.shape[1] <= 32 and r is not None:      # every channel of a pixel in one workgroup: the adjoint in the Winograd epilogue
        return ops.conv2d_wino_pnbwd(gz, u, ysaved, r, N, H, H, layer.c, slope)
    if u is not None:                              # wide layers: Winograd conv, then the (HBM-bound) adjoint kernel in place
        g = ops.conv2d_wino(gz, u, None, N, H, H, layer.c, 1.0)
        return ops.pixelnorm_lrelu_bwd(g, ysaved, r, slope, inplace=True)
    return ops.conv2d_pnbwd(gz, _wt(net, layer), ysaved, r, N, H, H, layer.ksize, layer.ksize - 1 - layer.pad, layer.c, slope)


# Weight gradients are leaves of the backward sweeps (nothing downstream reads them before the optimizer), so
# they are launched on a second HIP stream and overlap the backward-data chain on the main stream: two
# half-occupancy MFMA kernels share the CUs instead of running back to back.
# PGGAN_ASYNC_WGRAD=0 is the single-stream mode: the first thing to try when a missing cross-stream edge is suspected (bench.py toggles
# the attribute for its serial kernel timing).
ASYNC_WGRAD = os.environ.get('PGGAN_ASYNC_WGRAD', '1') != '0'
DERIVED_EVENT = True           # False: no completion event behind a refresh (ablation half of tests/test_e2e_gpu.py::test_derived_refresh_ordering only)
_SIDE = {}


# Every cross-stream ordering the step schedules issue goes through these three: plans._Recorder swaps them (module attributes of
# THIS module only -- never torch's classes, so stream / event traffic of other threads or libraries cannot leak into a plan).
def _wait_stream(waiter, other):
    waiter.wait_stream(other)


def _record_event(ev, stream):
    ev.record(stream)


def _wait_event(stream, ev):
    stream.wait_event(ev)


# Un-traced phase timeline (tools/phase_timeline.py): with ``PROBES`` set to a dict, the step schedules drop a timing event on the
# current stream at every phase boundary -- through ``_record_event``, so a launch plan re-records the same events on every replay and
# the probes cost ~25 event packets per step instead of the host slow-down of a tracer (rocprofv3 --kernel-trace makes the host the
# bottleneck of the 340-launch 1024^2 step: its "queue waiting" gaps are partly its own).  None (default): nothing is recorded.
PROBES = None


def probe(tag):
    if PROBES is not None:
        ev = torch.cuda.Event(enable_timing=True)
        _record_event(ev, torch.cuda.current_stream(torch._C._cuda_getDevice()))
        PROBES.setdefault(tag, []).append(ev)


def _side_stream():
    dev = torch.cuda.current_device()
    if dev not in _SIDE:
        _SIDE[dev] = torch.cuda.Stream(device=dev)
        ops._no_workspace_streams.add(_SIDE[dev].cuda_stream)      # (ops._stream_with_workspace: no sliced launch on it inside a capture)
    return _SIDE[dev]


class _on_side(object):
    """``with _on_side(t1, t2, ...):`` runs the body on the side stream after everything queued so far on
    the current stream; the tensors are registered with the allocator as in use on that stream."""

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if t is not None]
        self.active = ASYNC_WGRAD and len(self.tensors) > 0 and self.tensors[0].is_cuda

    def __enter__(self):
        if not self.active:
            return self
        main = torch.cuda.current_stream(torch._C._cuda_getDevice())      # explicit index: skips the slow device lookup
        self.side = _side_stream()
        _wait_stream(self.side, main)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if not self.active:
            return False
        self.ctx.__exit__(*exc)
        for t in self.tensors:
            t.record_stream(self.side)
        return False


def _join_side():
    """Main stream waits for every weight-gradient launch (call before the optimizer / all-reduce)."""
    if ASYNC_WGRAD and torch.cuda.is_available() and torch.cuda.current_device() in _SIDE:
        _wait_stream(torch.cuda.current_stream(torch._C._cuda_getDevice()), _SIDE[torch.cuda.current_device()])


def defer_to_side(net, fn):
    """Run ``fn()`` — the tail of a network's update: gradient all-reduce, Adam, derived weights — on the side stream,
    after everything queued so far on the current stream.  The current stream picks the result up in ``wait_pending``
    at its next use of the network's weights, so the tail of the D update overlaps the generator forward that opens
    the G step (the G step touches D only after G(z))."""
    if not (ASYNC_WGRAD and net._flat_param.is_cuda):
        fn()
        return
    main = torch.cuda.current_stream(torch._C._cuda_getDevice())
    side = _side_stream()
    side.wait_stream(main)
    rt = net._rt
    rt.defer_active = True
    try:
        with torch.cuda.stream(side):
            fn()
            ev = rt.take('pending_ev')                      # (_derived: the event behind Adam + the forward forms; the rest of the refresh follows it)
            if ev is None:
                ev = torch.cuda.Event()
                ev.record(side)
    finally:
        rt.defer_active = False
    rt.pending = ev


def wait_pending(net):
    """The current stream waits for a deferred update of ``net`` (no-op when there is none)."""
    ev = net._rt.pending
    if ev is not None:
        torch.cuda.current_stream(torch._C._cuda_getDevice()).wait_event(ev)
        net._rt.pending = None


def _grads_ready(net, layers):
    """Tell the gradient exchange (``parallel.GradExchange``, installed by ``Trainer`` as ``net._rt.grad_hook`` under data
    parallelism) that every weight-gradient launch of ``layers`` has been enqueued: their spans of the flat gradient
    buffer can start travelling while the sweep goes on."""
    hook = net._rt.grad_hook
    if hook is not None:
        for m in layers:                         # "complete" must never precede a deferred contribution that nothing carried
            if m._pending_wgrad is not None:
                _flush_wgrad(m)
        side = None
        if ASYNC_WGRAD and net._flat_param.is_cuda:
            side = _SIDE.get(torch.cuda.current_device())
        hook(layers, side)


# The gradient-penalty tangent term and the batched adjoint sweep both add to the weight gradient of every D layer.  For the
# Winograd layers the first contribution (3 images) is not launched on its own: it waits on the layer and rides in the launch of
# the second (pg_conv2d_wgrad_wino2_nhwc) -- one commit of dW instead of two, and the commit is a third of a 3-image launch.
DEFER_TANGENT_WGRAD = True     # False: reference half of tests/test_winograd.py::test_deferred_tangent_wgrad_matches_separate_launches


def _wino_wgrad_ok(layer, Hin):
    return (USE_WINOGRAD and layer.ksize == 3 and layer.pad == 1 and Hin >= 16 and not (Hin & (Hin - 1))
            and min(layer._gw.shape[2], layer._gw.shape[3]) >= _WINO_WGRAD_MIN_CHANNELS)


# The weight gradients of the entry (finest) block are the last and largest launches of the batched sweep: when the main stream finishes
# the sweep the second stream still has ~0.4 ms of them queued (tools/phase_timeline.py: D.wgrad_end - D.sweep_end at 1024^2), and with the
# G step's generator pass already done (EarlyG) the main stream has nothing to run until D's update is through.  The last
# one or two of them (fromRGB, then c1 of the entry block) are therefore launched on the main stream;
# the deferred update is ordered behind both streams (defer_to_side).  Not under a bucketed gradient exchange (its flushes wait for the
# second stream only).
# Same-box runs with the early generator pass on, ms per step, 0 | 1 | 2 launches on the main stream: 1024^2 10.182 | 10.135 | 10.134 and
# 10.185 | 10.118 | 10.076; 512^2 13.322 | 13.288 | 13.384.  Hence 2 at 1024^2, 1 at 512^2, none below (the 16-image stages keep both
# streams busy to the end).
def _tail_wgrad_on_main(H):
    return 2 if H >= 1024 else 1 if H >= 512 else 0


def _on_main(*tensors):
    return _contextlib.nullcontext()


def _wgrad(x, gz, layer, N, Hin, bias=True, ups=False, defer=False, on_main=False):
    """Weight (and bias) gradient of one conv layer on the side stream.  The wide 3x3 layers take the Winograd form
    (2.25x fewer MFMAs, 1.3-1.7x faster from 16x16 up, 16-channel sides included); the 8-channel layers and the
    4x4 / 8x8 maps keep the direct kernels.  ``defer``: a bias-free contribution that a later ``_wgrad`` of the same layer
    (same step, same input geometry) will carry along."""
    wino = _wino_wgrad_ok(layer, Hin)
    if defer and wino and DEFER_TANGENT_WGRAD and not bias and not ups:
        layer._pending_wgrad = (x, gz, N, Hin)
        return
    pend = layer._pending_wgrad
    if pend is not None and not (wino and pend[3] == Hin and not ups):
        _flush_wgrad(layer)
        pend = None
    layer._pending_wgrad = None
    with (_on_main if on_main else _on_side)(x, gz, *(pend[:2] if pend is not None else ())):
        if wino:
            ops.conv2d_wgrad_wino(x, gz, layer._gw, layer._gb if bias else None, N, Hin, Hin, layer.c, ups=ups,
                                  second=(pend[0], pend[1], pend[2], False) if pend is not None else None)
            return
        ops.conv2d_wgrad(x, gz, layer._gw, layer._gb if bias else None, N, Hin, Hin, layer.ksize, layer.pad,
                         layer.c, ups=ups)


def _flush_wgrad(layer):
    """Launch a deferred contribution on its own (nothing came to carry it)."""
    pend = layer._pending_wgrad
    if pend is None:
        return
    layer._pending_wgrad = None
    x, gz, N, Hin = pend
    with _on_side(x, gz):
        ops.conv2d_wgrad_wino(x, gz, layer._gw, None, N, Hin, Hin, layer.c)


_ONES = {}


def _ones(n, device):
    key = (n, str(device))
    if key not in _ONES:
        _ONES[key] = torch.ones(n, device=device, dtype=torch.float32)
    return _ONES[key]


# ------------------------------------------------------------------------------------------
# Generator
# ------------------------------------------------------------------------------------------
def generator_forward(G, z, save=False, out=None, pair_out=None):
    """reference network.py:118-139.  z [N,latent] -> NCHW image [N,C,r,r] (written into ``out``).  ``pair_out`` = (outA, outB or None):
    the two halves of the batch go to two image buffers (the paired D-step / G-step pass, ``_generator_pair``); returns (imgA, imgB)."""
    wait_pending(G)
    ops.require_gpu()
    G._sync_version()                 # also notice torch-side updates (torch.optim.*, load_state_dict) before any derived weight is used
    z = _check_dev(z, 'latents')
    N, L = z.shape
    if L != G.latent_size or L % 4:
        raise ValueError('latent size %d (expected %d, multiple of 4)' % (L, G.latent_size))
    depth, alpha = int(G.depth), float(G.alpha)
    C = G.num_channels
    b0 = G.block0
    G._ensure_buffers()
    ctx = saved.GContext(N=N, depth=depth, alpha=alpha, recs=[])
    if G.normalize_latents:
        zn, _ = ops.pixelnorm_fwd(z, G.eps)                                   # :120-123
    else:
        zn = z
    ctx.zn = zn

    def layer(x, lay, H, ups=False):
        if lay.pixelnorm:
            u = _wino(lay, N, H, lay.conv.weight.shape[2]) if lay.ksize == 3 else None
            if u is not None and u.shape[1] <= 32:   # all couts of a pixel in one workgroup: PixelNorm in the Winograd epilogue
                return ops.conv2d_wino_pixelnorm(x, u, lay.conv.bias.data, N, H, H, lay.c, lay.slope, lay.eps, ups=ups)
            if u is not None:                     # wide layers: Winograd conv, PixelNorm as its own (HBM-bound) pass
                y = ops.conv2d_wino(x, u, lay.conv.bias.data, N, H, H, lay.c, lay.slope, ups=ups)
                return ops.pixelnorm_fwd(y, lay.eps, inplace=True)
            # conv + bias + act + PixelNorm in one launch where the tile allows it
            return ops.conv2d_pixelnorm(x, lay.conv.weight.data, lay.conv.bias.data, N, H, H, lay.ksize, lay.pad, lay.c,
                                        lay.slope, lay.eps, ups=ups)
        return _conv(x, lay, N, H, ups=ups), None

    y1, r1 = layer(zn.view(N, 1, 1, L), b0.c1, 1)                            # 4x4 conv pad 3 on 1x1
    y2, r2 = layer(y1, b0.c2, 4)
    ctx.y1, ctx.r1, ctx.y2, ctx.r2 = y1, r1, y2, r2
    def to_rgb(h, t, H, out_mul=1.0, prev=None, prev_mul=0.0):
        if pair_out is None:
            return ops.torgb_fwd(h, t.conv.weight.data, t.conv.bias.data, N, C, H, H, t.c, out_mul=out_mul, prev=prev, prev_mul=prev_mul, out=out)
        n2 = N // 2
        return tuple(ops.torgb_fwd(h[a:b], t.conv.weight.data, t.conv.bias.data, n2, C, H, H, t.c, out_mul=out_mul,
                                   prev=prev[a:b] if prev is not None else None, prev_mul=prev_mul, out=o)
                     for (a, b), o in zip(((0, n2), (n2, N)), pair_out))
    if depth == 0:
        img = to_rgb(y2, b0.toRGB, 4)                                          # :55-56
        return (img, ctx) if save else img
    h, H = y2, 4
    for i in range(depth):                                                    # :126-130
        blk = G.blocks[i]
        H *= 2
        a1, ra1 = layer(h, blk.c1, H, ups=True)                               # upsample fused into the conv
        img = None
        if (i == depth - 1 and alpha >= 1.0 and pair_out is None and blk.c2.pixelnorm and blk.c2.ksize == 3 and a1.is_cuda
                and _wino(blk.c2, N, H, blk.c2.conv.weight.shape[2]) is None):
            t = blk.toRGB                          # the last conv writes the image too (toRGB in its epilogue: the 1024^2 stage)
            try:
                a2, ra2, img = ops.conv2d_pixelnorm_torgb(a1, blk.c2.conv.weight.data, blk.c2.conv.bias.data, t.conv.weight.data, t.conv.bias.data,
                                                          N, C, H, H, blk.c2.c, blk.c2.slope, t.c, blk.c2.eps, out=out)
            except ops.Unsupported:
                FALLBACKS['toRGB in the epilogue %dx%d' % (H, H)] += 1
                img = None
        if img is None:
            a2, ra2 = layer(a1, blk.c2, H)
        ctx.recs.append(saved.GBlock(blk=blk, inp=h, a1=a1, r1=ra1, a2=a2, r2=ra2, H=H))
        hprev, h = h, a2
    if img is not None:
        return (img, ctx) if save else img
    t, pt = G.rgb_heads(depth, alpha)
    prev = None
    if pt is not None:                                                        # :131-135
        prev = ops.torgb_fwd(hprev, pt.conv.weight.data, pt.conv.bias.data, N, C, H // 2, H // 2, pt.c)
    img = to_rgb(h, t, H, out_mul=alpha, prev=prev, prev_mul=1.0 - alpha)    # :138
    return (img, ctx) if save else img


def generator_backward(G, ctx, g_out):
    """Adjoint sweep of generator_forward: accumulates into G's flat gradient buffer."""
    wait_pending(G)
    G._ensure_buffers()
    N, depth, alpha = ctx.N, ctx.depth, ctx.alpha
    C = G.num_channels
    b0 = G.block0
    active = [b0.c1, b0.c2]
    g_extra = None
    top_done = False
    t, pt = G.rgb_heads(depth, alpha)
    if depth == 0:
        with _on_side(g_out, ctx.y2):
            ops.torgb_wgrad(g_out, ctx.y2, t._gw, t._gb, N, C, 4, 4, t.c, 1.0)
        g = ops.torgb_bwd_data(g_out, t.conv.weight.data, N, C, 4, 4, t.c)
        active.append(t)
    else:
        rec = ctx.recs[-1]
        H = rec.H
        with _on_side(g_out, rec.a2):
            ops.torgb_wgrad(g_out, rec.a2, t._gw, t._gb, N, C, H, H, alpha * t.c, alpha)
        # toRGB's adjoint + the adjoint of the top block's last (LeakyReLU -> PixelNorm) in one launch (network.py:138, :44-52)
        if rec.r2 is not None:
            g = ops.torgb_bwd_data_pnbwd(g_out, t.conv.weight.data, rec.a2, rec.r2, N, C, H, H, alpha * t.c, rec.blk.c2.slope)
            top_done = True
        else:                                         # (a generator built without PixelNorm: the adjoint is LeakyReLU' alone)
            g = ops.torgb_bwd_data(g_out, t.conv.weight.data, N, C, H, H, alpha * t.c)
        active.append(t)
        if pt is not None:
            with _on_side(g_out, rec.inp):
                ops.torgb_wgrad(g_out, rec.inp, pt._gw, pt._gb, N, C, H // 2, H // 2, (1 - alpha) * pt.c,
                                1 - alpha, down=True)
            g_extra = ops.torgb_bwd_data(g_out, pt.conv.weight.data, N, C, H // 2, H // 2, (1 - alpha) * pt.c, down=True)
            active.append(pt)
    _grads_ready(G, active[2:])
    recs = ctx.recs
    for k in range(len(recs) - 1, -1, -1):
        rec = recs[k]
        blk, H = rec.blk, rec.H
        c1, c2 = blk.c1, blk.c2
        if top_done:                                  # (the top block's adjoint came with toRGB's)
            gz2, top_done = g, False
        else:
            gz2 = ops.pixelnorm_lrelu_bwd(g, rec.a2, rec.r2, c2.slope, inplace=True)
        _wgrad(rec.a1, gz2, c2, N, H)
        # backward-data conv of c2 + adjoint of c1's (LeakyReLU -> PixelNorm) in one launch
        gz1 = _dgrad_pnbwd(G, gz2, c2, N, H, rec.a1, rec.r1, c1.slope)
        _wgrad(rec.inp, gz1, c1, N, H, ups=True)
        # backward-data conv of c1 + adjoint of the nearest x2 upsample (sum over 2x2 = 4 * average pool, exact in fp32)
        # + the fade-in branch's gradient, all in the conv epilogue
        # ... and, where it fits, the adjoint of the coarser block's last (LeakyReLU -> PixelNorm) as well
        prev = (recs[k - 1].a2, recs[k - 1].r2, recs[k - 1].blk.c2.slope) if k > 0 else (ctx.y2, ctx.r2, b0.c2.slope)
        g, top_done = _dgrad_pool(G, gz1, c1, N, H, other=g_extra, a=4.0, b=1.0, pnb=prev)
        g_extra = None
        active += [c1, c2]
        _grads_ready(G, [c1, c2])
    gz2 = g if top_done else ops.pixelnorm_lrelu_bwd(g, ctx.y2, ctx.r2, b0.c2.slope, inplace=True)
    _wgrad(ctx.y1, gz2, b0.c2, N, 4)
    g1 = _dgrad(G, gz2, b0.c2, N, 4)
    gz1 = ops.pixelnorm_lrelu_bwd(g1, ctx.y1, ctx.r1, b0.c1.slope, inplace=True)
    _wgrad(ctx.zn.view(N, 1, 1, -1), gz1, b0.c1, N, 1)
    _grads_ready(G, [b0.c1, b0.c2])
    return active


# ------------------------------------------------------------------------------------------
# Minibatch stddev: local-shard (default) or exact-global under data parallelism
# ------------------------------------------------------------------------------------------
# Default under data parallelism: every rank evaluates reference network.py:174-187 on its OWN minibatch (per-rank parity
# with the single-GPU reference at batch mb is exact).  ``Trainer(parallel=dp, global_stddev=True)`` switches to the exact-global mode:
# the one scalar a group's statistic is (and the three scalars its adjoint / Hessian-vector term need: G_sigma, <v, x - mu>, mean v) are
# reduced over all ranks, so world x mb equals one process at batch world * mb.  The collectives are a few floats each on the main
# stream, in the same order on every rank; steps are launched eagerly in this mode (wgan_gp_loss: no hipGraph / launch plan).
def _mbstd_fwd(D, x, groups, cp):
    dp = D._rt.global_stddev
    if dp is None:
        return ops.mbstd_fwd(x, groups, cp)
    # the split kernels take the element count of the whole group as local count x ranks (csrc/elementwise.hip mbstd_write_kernel):
    # equal per-rank batches are part of the mode's contract -- checked here, once per batch shape (it was only claimed)
    if D._rt.gs_checked != (int(x.shape[0]), groups):
        dp.assert_same_on_all_ranks(int(x.shape[0]) // groups, 'exact-global minibatch stddev: the per-rank minibatch size')
        D._rt.gs_checked = (int(x.shape[0]), groups)
    st = ops.mbstd_stats(x, groups)
    return ops.mbstd_write(x, st, dp.all_gather_rows(st), cp)


def _mbstd_tangent(D, x, tx, stats, cp):
    dp = D._rt.global_stddev
    if dp is None:
        return ops.mbstd_tangent(x, tx, stats, cp)
    ts = ops.mbstd_tangent_stats(x, tx, stats)
    return ops.mbstd_tangent_write(tx, ts, dp.all_gather_rows(ts), stats, cp)


def _mbstd_bwd(D, gy, x, stats, cp, apply_mask, mask_slope, tx=None, tstats=None, gy_first=None, out=None):
    dp = D._rt.global_stddev
    if dp is None:
        return ops.mbstd_bwd(gy, x, stats, cp, apply_mask, mask_slope, tx=tx, tstats=tstats, gy_first=gy_first, out=out)
    gs = ops.mbstd_gsum(gy, gy_first if tx is not None else None, stats.shape[0], tuple(x.shape), cp)
    dp.all_reduce_flat(gs.view(-1))
    return ops.mbstd_bwd_global(gy, x, stats, cp, apply_mask, gs, dp.world_size, mask_slope, tx=tx, tstats=tstats, gy_first=gy_first, out=out)


def _mbstd_bwd_hvp(D, g_head, g_mixed, rec, hvp, fr_slope):
    """Minibatch-stddev adjoint of the last block ``rec`` under the gradient penalty: the head images take ``g_head``; the mixed images behind
    them (one extra group) take ``g_mixed`` (None: they have no first-order gradient) plus the Hessian-vector injection of ``hvp``."""
    nh, inp, stats, cp = hvp.n_head, rec.inp, rec.stats, rec.blk.c1.cin_store
    gin = torch.empty_like(inp)
    ng = stats.shape[0] - 1
    _mbstd_bwd(D, g_head, inp[:nh], stats[:ng], cp, rec.first, fr_slope, out=gin[:nh])
    _mbstd_bwd(D, g_mixed, inp[nh:], stats[ng:], cp, rec.first, fr_slope, tx=hvp.tx, tstats=hvp.tstats, gy_first=hvp.gy_first, out=gin[nh:])
    return gin


# ------------------------------------------------------------------------------------------
# Discriminator
# ------------------------------------------------------------------------------------------
# The G step's pass through D is followed by a backward-data sweep only (no weight gradients of D): the fp32 output of the entry block's
# fromRGB layer is then needed by nobody but the block's first conv, which evaluates it in its gather from the image
# (ops.conv2d_fromrgb: 12 B of image per pixel instead of 32 B written by one launch and read by the next; the 1024^2 stage).
# In the backward sweeps fromRGB's backward-data, and in the batched adjoint sweep its weight gradient too, ride in the epilogue of the entry
# block's backward-data conv (ops.conv2d_masked_fromrgb_bwd: the 8-channel gradient is then never written); the generator's last conv
# writes the image in its epilogue (ops.conv2d_pixelnorm_torgb).  The unfused launches are the path of every other shape, of alpha < 1,
# of a bucketed gradient exchange, and the fallback when a fused launch answers ``ops.Unsupported``.
def d_forward(D, x, groups=1, keep_input=True):
    """reference network.py:225-240 on a batch of ``groups`` independent minibatches stacked along
    N (minibatch-stddev is evaluated per group).  Returns (scores [NB], ctx with every activation).
    ``keep_input=False``: the caller will not ask for D's weight gradients (``d_backward(full=False)``) -- the entry block's fromRGB
    output may stay unmaterialised (``rec.inp`` is None then; its sign bytes ``rec.inpb`` are always there)."""
    wait_pending(D)
    D._sync_version()
    NB, C, r, _ = x.shape
    depth, alpha = int(D.depth), float(D.alpha)
    if r != 4 * 2 ** depth or C != D.num_channels:
        raise ValueError('input %s does not match depth %d / %d channels' % (tuple(x.shape), depth, D.num_channels))
    nb = len(D.blocks)
    e = nb - 1 - depth                                                        # blocks[-(depth+1)]  (:227)
    D._ensure_buffers()
    ctx = saved.DContext(NB=NB, groups=groups, depth=depth, alpha=alpha, x=x, recs=[])
    pn = bool(getattr(D, 'pixelnorm', False))
    fr = D.blocks[e].fromRGB
    sb = USE_SIGN_BYTES and not pn                                            # byte copies of the fp32 activations (masks)
    curb = None
    fused = None                                 # (a1, a1b) of the entry block when its c1 ran with fromRGB in the gather
    if not keep_input and sb and r >= SIGN_BYTES_MIN_H and e < nb - 1 and x.is_cuda:
        c1 = D.blocks[e].c1
        if c1.ksize == 3 and c1.pad == 1 and _wino(c1, NB, r, c1.conv.weight.shape[2]) is None:
            try:
                a1, a1b, curb = ops.conv2d_fromrgb(x, fr.conv.weight.data, fr.conv.bias.data, fr.c, fr.slope, c1.conv.weight.data,
                                                   c1.conv.bias.data, NB, C, r, r, c1.c, c1.slope)
                fused, cur = (a1, a1b), None
            except ops.Unsupported:
                FALLBACKS['fromRGB in the gather %dx%d' % (r, r)] += 1
    if fused is None:
        cur = ops.fromrgb_fwd(x, fr.conv.weight.data, fr.conv.bias.data, NB, C, r, r, fr.c, fr.slope, signs_out=sb and r >= SIGN_BYTES_MIN_H)
        if sb and r >= SIGN_BYTES_MIN_H:
            cur, curb = cur
    H = r
    a2 = None
    for k, j in enumerate(range(e, nb)):
        blk = D.blocks[j]
        last = (j == nb - 1)
        rec = saved.DBlock(blk=blk, inp=cur, H=H, first=(k == 0), last=last, inpb=curb if k == 0 else None)
        if last:
            mb, stats = _mbstd_fwd(D, cur, groups, blk.c1.cin_store)          # :168
            a1 = _conv(mb, blk.c1, NB, H)
            if pn:
                a1, rec.r1 = ops.pixelnorm_fwd(a1, inplace=True)
            a2 = _conv(a1, blk.c2, NB, H)                                     # 4x4 pad 0 -> 1x1
            if pn:
                a2, rec.r2 = ops.pixelnorm_fwd(a2, inplace=True)
            rec.mb, rec.stats, rec.a1, rec.a2 = mb, stats, a1, a2
        else:
            if k == 0 and fused is not None:
                a1, rec.a1b = fused
            elif sb and H >= SIGN_BYTES_MIN_H:
                a1, rec.a1b = _conv(cur, blk.c1, NB, H, signs_out=True)
            else:
                a1 = _conv(cur, blk.c1, NB, H)
            if pn:                                                            # a1/a2 hold the NORMALISED outputs
                a1, rec.r1 = ops.pixelnorm_fwd(a1, inplace=True)
            pf = None
            if k == 0 and alpha < 1.0:                                        # :230-233
                nfr = D.blocks[j + 1].fromRGB
                pf = rec.pf = ops.fromrgb_fwd(x, nfr.conv.weight.data, nfr.conv.bias.data, NB, C, H // 2, H // 2,
                                              nfr.c, nfr.slope, pool=True)
            pa, pb = (alpha, 1.0 - alpha) if pf is not None else (1.0, 0.0)
            if pn:
                a2 = _conv(a1, blk.c2, NB, H)
                a2, rec.r2 = ops.pixelnorm_fwd(a2, inplace=True)
                cur = ops.avgpool2_fwd(a2, pf, pa, pb)                        # :229,238
            else:                                                             # pool (+ fade-in blend) in the conv epilogue
                a2, cur = _conv_pool(a1, blk.c2, NB, H, other=pf, a=pa, b=pb, y_bytes=USE_SIGN_BYTES and H >= SIGN_BYTES_MIN_H)
            rec.a1, rec.a2 = a1, a2
            H //= 2
        ctx.recs.append(rec)
    s = ops.linear1_fwd(a2, D.linear.weight.data, D.linear.bias.data)         # :239
    return s, ctx


# ---- three-pass forward of a D step: the real, fake and mixed thirds of the [real | fake | mixed] batch as three passes -----------------
# All three passes write into ONE set of batched activation tensors (ops.Arena), so the adjoint sweeps stay batched over all 3N images.
class _DForwardBuffers(object):
    """Buffers of the three-pass D forward, kept per (network, stage, shape) -- launch plans bake their addresses: the image buffer
    [3N,C,r,r] and the arena with the batched activations."""

    def __init__(self):
        self.arena = ops.Arena()
        self.x3 = None
        self.g_out = None                   # [N,C,r,r] scratch G(z) is written to when the step augments (the fake third is its augmented form)
        self.key = None
        self.owner = None                   # weakref to the _ArenaUse token of the D-loss state whose activations live in these buffers


class _ArenaUse(object):
    """Token a D-loss state holds while its saved activations alias the per-network arena: as long as the state is alive and its
    ``backward()`` has not run, another D-loss forward on the same network must not write into those buffers (it allocates fresh
    tensors instead -- two losses then backward, a validation loss between forward and backward)."""
    __slots__ = ('consumed', '__weakref__')

    def __init__(self):
        self.consumed = False


def _arena_free(st):
    tok = st.owner() if st.owner is not None else None
    return tok is None or tok.consumed


def _lazy_unpool_ok(rec, save_adjoints):
    """May the pool adjoint behind block ``rec`` stay un-evaluated, for the consumers of the block's c2 gradient to apply in their gathers
    (ops.conv2d_unpooled / conv2d_wgrad_unpooled)?  Needs c2's output as sign bytes and the 8-channel 3x3 layers those kernels are built for."""
    if not (USE_LAZY_UNPOOL and not save_adjoints and rec.H % 32 == 0 and rec.a2.dtype == torch.uint8):     # (the cheap tests first)
        return False
    c2 = rec.blk.c2
    w = c2.conv.weight.shape
    return w[3] == 8 and w[2] in (8, 16) and c2.ksize == 3


# ---- the adjoint sweep: d_backward drives it; one step per thing that happens to a block ---------------------------------------------
#   _consume | _pn_adjoints   hand-over of the coarser block (saved.PoolAdjoint) -> gz2, gz1 (+ c2's weight gradient)
#   _hand_over                c1's backward-data conv + the pool adjoint -> the hand-over to the finer block (+ _fade_in at the boundary)
#   _entry                    c1's backward-data conv of the entry block, fromRGB's gradients, the image gradient
def _consume(D, hand, rec, n, full):
    """c2 of block ``rec`` over ``n`` images: (gz2, gz1) and c2's weight gradient from what the coarser block handed over.  A lazy
    hand-over is unpooled in the gathers of its two consumers (gz2 is never written: None); when they answer ``ops.Unsupported`` it is
    evaluated after all."""
    c2, H = rec.blk.c2, rec.H
    a1 = saved.Sign.a1(rec, n if rec.last else None)

    def lazy(up, _):
        if up is not hand.up.bytes:                # the redo: the pool adjoint as a launch of its own, c2's own launches below
            return ops.avgpool2_bwd(hand.coarse, up, 4.0 * hand.mul, hand.up.slope), None
        gz1 = ops.conv2d_unpooled(hand.coarse, _wt(D, c2), up, hand.mul, hand.up.slope, n, H, H, c2.c,
                                  mask=a1.bytes if a1.bytes is not None else a1.f32, mask_slope=a1.slope)
        if full:
            _flush_wgrad(c2)                       # (this launch does not go through _wgrad: a deferred tangent term rides nowhere)
            with _on_side(a1.f32, hand.coarse, up):
                ops.conv2d_wgrad_unpooled(a1.f32, hand.coarse, up, hand.mul, hand.up.slope, c2._gw, c2._gb, n, H, H, c2.c)
        return None, gz1                           # (shape checks are identical for both entry points: nothing was accumulated on failure)
    gz2, gz1 = (hand.g, None) if hand.g is not None else _bytes_first(lazy, hand.up, lambda: 'lazy unpool %dx%d' % (H, H))
    if gz1 is None:
        if full:
            _wgrad(a1.f32, gz2, c2, n, H)
        gz1 = _dgrad(D, gz2, c2, n, 1 if rec.last else H, a1)
    return gz2, gz1


_NO_INJECTION = saved.PNInjection()


def _pn_bwd(gy, y, r, slope, nh, inj):
    """(LeakyReLU -> PixelNorm) adjoint on a batch whose images [nh:] additionally receive the
    gradient-penalty Hessian-vector injection ``inj`` (None: plain adjoint on the whole batch)."""
    if inj is None:
        return ops.pixelnorm_lrelu_bwd(gy, y, r, slope, inplace=True)
    per = r.numel() // y.shape[0]
    if nh > 0:
        ops.pixelnorm_lrelu_bwd(gy[:nh], y[:nh], r[:nh * per], slope, inplace=True)
    ops.pixelnorm_lrelu_bwd(gy[nh:], y[nh:], r[nh * per:], slope, inj=inj, out=gy[nh:])
    return gy


def _pn_head_seed(D, gscore, a2, nh):
    """The head of the PixelNorm discriminator's sweep: the adjoint wrt the NORMALISED ``a2`` (no mask), the mixed images [nh:] with
    a zero score gradient (they take injections only)."""
    g = ops.linear1_bwd_data(gscore, D.linear.weight.data, None, (nh,) + tuple(a2.shape[1:]))
    if nh < a2.shape[0]:
        gtop, g = g, torch.empty_like(a2)            # (C-ABI launches, not ATen ops: a launch plan replays only those)
        ops.zero_(g[nh:])
        ops.axpby_mask(gtop, a=1.0, out=g[:nh])
    return g


def _pn_adjoints(D, hand, rec, n, nh, full, adj, inj):
    """``_consume`` for Discriminator(pixelnorm=True): every c1/c2 is conv -> LeakyReLU -> PixelNorm (network.py:32-41), so the masks
    can no longer be fused into the backward-data convs; the adjoint of each (LeakyReLU, PixelNorm) pair is one ``pixelnorm_lrelu_bwd``
    launch, which on the mixed images [nh:] adds the PixelNorm Hessian-vector injections ``inj``.  ``adj`` takes copies of gy2 / gy1."""
    c1, c2, H = rec.blk.c1, rec.blk.c2, rec.H
    if adj is not None:
        adj.gy2 = ops.axpby_mask(hand.g, a=1.0)              # device copy through the C-ABI (recorded by a launch plan)
    gz2 = _pn_bwd(hand.g, rec.a2, rec.r2, c2.slope, nh, inj.inj2)
    if full:
        _wgrad(rec.a1, gz2, c2, n, H)
    gy1 = _dgrad(D, gz2, c2, n, 1 if rec.last else H)
    if adj is not None:
        adj.gy1 = ops.axpby_mask(gy1, a=1.0)
    return gz2, _pn_bwd(gy1, rec.a1, rec.r1, c1.slope, nh, inj.inj1)


def _fade_in(D, ctx, rec, prev, gin, full, adj):
    """The fade-in branch behind the entry block (network.py:230-233): the adjoint of ``rec``'s fromRGB of the pooled image from the coarse
    gradient ``gin`` (x (1 - alpha), x LeakyReLU' of the entry block ``prev``'s pf), and that layer's weight gradient.  Returns (gpf, the layer) for ``_entry`` to add to the image gradient."""
    pfr = rec.blk.fromRGB                                   # the block whose fromRGB fed the fade-in
    x, H = ctx.x, rec.H
    gpf = ops.axpby_mask(gin, mask=prev.pf, a=1.0 - ctx.alpha, mask_slope=pfr.slope)
    if adj is not None:
        adj.gpf = gpf
    if full:
        with _on_side(gpf, x):
            ops.fromrgb_wgrad(gpf, x, pfr._gw, pfr._gb, ctx.NB, D.num_channels, H, H, pfr.c, pool=True)
    return gpf, pfr


def _hand_over(D, ctx, rec, prev, gz1, gin, full, adj, pn):
    """What block ``rec`` hands to the finer block ``prev``: c1's backward-data conv (``gin`` None; the 4x4 block comes with its input
    adjoint) and the pool adjoint -- in one launch, left lazy for prev's c2 consumers, or as two launches; at the fade-in boundary
    x alpha, with the fade-in branch beside it.  Returns (saved.PoolAdjoint, ``_fade_in``'s result or None).  ``adj``: prev's DAdjoint."""
    c1, H, NB = rec.blk.c1, rec.H, ctx.NB
    fade = prev.first and ctx.alpha < 1.0
    mul = ctx.alpha if fade else 1.0
    up = None if pn else saved.Sign.a2(prev)                # (PixelNorm: the adjoint wrt the NORMALISED a2, no mask)
    lazy = not pn and (gin is None or fade) and _lazy_unpool_ok(prev, adj is not None)    # (the 4x4 block's own hand-over is never lazy)
    if gin is None and not (fade or lazy or pn):
        # backward-data conv + pool adjoint + LeakyReLU' of the finer block's output in one kernel
        return saved.PoolAdjoint(g=_dgrad_unpool(D, gz1, c1, NB, H, up, 1.0)), None
    if gin is None:
        gin = _dgrad(D, gz1, c1, NB, H)
    if lazy:
        # plain coarse gradient; the finer block's c2 consumers apply the pool adjoint in their gathers instead of reading a fine-resolution
        # gradient (604 MB at the 1024^2 stage) -- across the fade-in boundary too (x alpha, round 4)
        hand = saved.PoolAdjoint(coarse=gin, up=up, mul=0.25 * mul)
    elif pn:
        hand = saved.PoolAdjoint(g=ops.avgpool2_bwd(gin, None, mul))
    else:
        hand = saved.PoolAdjoint(g=ops.avgpool2_bwd(gin, _f32(up), mul, up.slope))
    return hand, (_fade_in(D, ctx, rec, prev, gin, full, adj) if fade else None)


def _entry(D, ctx, rec, gz1, gin, full, want_gimg, adj, faded, tail, pn):
    """The entry block's end of the sweep: gf, the adjoint of fromRGB's pre-activation (``gin`` None: c1's backward-data conv is still to
    run; at depth 0 the minibatch-stddev adjoint came with it), fromRGB's weight gradient and, with ``want_gimg``, the image gradient
    (returned) including the fade-in branch's (``faded``).  Where the shape allows -- never under PixelNorm (``pn``), whose adjoints are
    not masked convs -- fromRGB's backward-data and its weight gradient ride in the epilogue of c1's backward-data conv."""
    blk, H, NB, x, C = rec.blk, rec.H, ctx.NB, ctx.x, D.num_channels
    c1, fr = blk.c1, blk.fromRGB
    gimg = None
    fused = fw_fused = False           # the backward-data conv wrote the image gradient / accumulated fromRGB's weight gradient itself
    # fromRGB's weight gradient rides in the same epilogue when the sweep asks for weight gradients -- not under a bucketed
    # gradient exchange, whose flushes wait for the weight-gradient stream only (as the tail launches on the main stream)
    fw = full and D._rt.grad_hook is None
    if (not pn and gin is None and (want_gimg or fw) and rec.inpb is not None and x.is_cuda and c1.ksize == 3 and c1.pad == 1
            and _wino(c1, NB, H, c1.conv.weight.shape[3], transposed=True) is None):
        # the 8-channel gradient itself is written only when somebody reads it afterwards (the tangent term of the gradient penalty)
        try:
            gin, gimg = ops.conv2d_masked_fromrgb_bwd(gz1, _wt(D, c1), rec.inpb, fr.slope, fr.conv.weight.data, fr.c, NB, C, H, H, c1.c,
                                                      keep_gf=adj is not None or (full and not fw), want_gimg=want_gimg,
                                                      img=x if fw else None, rgb_dw=fr._gw if fw else None, rgb_db=fr._gb if fw else None)
            fused, fw_fused = True, fw
        except ops.Unsupported:
            FALLBACKS['fromRGB adjoint in the epilogue %dx%d' % (H, H)] += 1
    if gin is None and not fused:
        gin = _dgrad(D, gz1, c1, NB, H, saved.Sign.inp(rec))
    if adj is not None:
        adj.gf = gin
    if full and not fw_fused:
        with (_on_main if tail >= 1 else _on_side)(gin, x):
            ops.fromrgb_wgrad(gin, x, fr._gw, fr._gb, NB, C, H, H, fr.c)
    if not want_gimg:
        return None
    if not fused:
        gimg = torch.empty_like(x)
        ops.fromrgb_bwd_data(gin, fr.conv.weight.data, gimg, NB, C, H, H, fr.c)
    if faded is not None:
        gpf, pfr = faded
        ops.fromrgb_bwd_data(gpf, pfr.conv.weight.data, gimg, NB, C, H // 2, H // 2, pfr.c, pool=True, accumulate=True)
    return gimg


def d_backward(D, ctx, gscore, full, want_gimg, save_adjoints=False, hvp=None):
    """First-order adjoint sweep through D for the batch in ``ctx``.

    gscore [NB] : d loss / d score.   full: also accumulate weight/bias gradients.
    want_gimg   : return d loss / d input image (NCHW).
    hvp         : saved.Hvp — the last ``NB-n_head`` images form one extra group
                  whose score gradient is zero and which only receives the minibatch-stddev
                  Hessian-vector injection (and, in a PixelNorm discriminator, the per-layer
                  injections ``hvp.injs``); ``gscore`` then has n_head entries."""
    wait_pending(D)
    D._ensure_buffers()
    pn = bool(getattr(D, 'pixelnorm', False))
    NB, alpha, recs = ctx.NB, ctx.alpha, ctx.recs
    adj = [saved.DAdjoint() for _ in recs] if save_adjoints else [None] * len(recs)
    nh = NB if hvp is None else hvp.n_head
    injs = hvp.injs if pn and hvp is not None else None
    n4 = NB if pn else nh                                    # images the 4x4 block's convs run over (PixelNorm: the mixed ones take injections there)
    a2 = recs[-1].a2
    tail = _tail_wgrad_on_main(recs[0].H) if (full and not pn and ASYNC_WGRAD and D._rt.grad_hook is None and len(recs) > 1) else 0
    if full and not pn:
        ops.linear1_wgrad(gscore, a2[:nh], D._lin_gw, D._lin_gb)
    hand = saved.PoolAdjoint(g=_pn_head_seed(D, gscore, a2, nh) if pn else ops.linear1_bwd_data(
        gscore, D.linear.weight.data, a2[:nh], (nh,) + tuple(a2.shape[1:]), recs[-1].blk.c2.slope))
    if full and pn:                                  # (behind the seed: the order this sweep has always issued them in)
        ops.linear1_wgrad(gscore, a2[:nh], D._lin_gw, D._lin_gb)
    gimg = faded = None
    for idx in range(len(recs) - 1, -1, -1):
        rec = recs[idx]
        c1, H = rec.blk.c1, rec.H
        n = n4 if rec.last else NB
        if pn:
            gz2, gz1 = _pn_adjoints(D, hand, rec, n, nh, full, adj[idx], injs[idx] if injs is not None else _NO_INJECTION)
        else:
            gz2, gz1 = _consume(D, hand, rec, n, full)
        if full:
            _wgrad(rec.mb[:n] if rec.last else rec.inp, gz1, c1, n, H, on_main=rec.first and not rec.last and tail >= 2)
        gin = None
        if rec.last:
            gmb = _dgrad(D, gz1, c1, n, H)                                    # [n,4,4,CP]
            if hvp is None:
                gin = _mbstd_bwd(D, gmb, rec.inp, rec.stats, c1.cin_store, rec.first, rec.blk.fromRGB.slope)
            else:
                gin = _mbstd_bwd_hvp(D, gmb[:nh], gmb[nh:] if pn else None, rec, hvp, rec.blk.fromRGB.slope)
        if save_adjoints:
            adj[idx].gz2, adj[idx].gz1 = gz2, gz1
            if rec.last:
                adj[idx].gmb = gmb
        if rec.first:
            gimg = _entry(D, ctx, rec, gz1, gin, full, want_gimg, adj[idx], faded, tail, pn)
        else:
            hand, faded = _hand_over(D, ctx, rec, recs[idx - 1], gz1, gin, full, adj[idx - 1], pn)
        if full:
            _grads_ready(D, _d_block_done(D, recs, idx, alpha))
    return gimg, (adj if save_adjoints else None)


def _d_block_done(D, recs, idx, alpha):
    """Layers whose weight gradients are complete once block ``idx`` of the batched backward sweep has been processed
    (the tangent pass ran before the sweep, so nothing else accumulates into them)."""
    rec = recs[idx]
    blk = rec.blk
    done = [blk.c1, blk.c2]
    if rec.last:
        done.append(D._lin_layer)
    if rec.first or (recs[idx - 1].first and alpha < 1.0):
        done.append(blk.fromRGB)                 # the entry block's fromRGB / the fade-in branch's fromRGB
    return done


def d_tangent_wgrad(D, sub, adj, u):
    """Gradient-penalty second-order term, steps (i)+(ii): push the seed ``u`` (NCHW, same shape as the
    mixed batch) through the masked linear maps of D and accumulate, per layer,
    dW += c * wgrad(tangent_input, first_backward_adjoint).  ``adj``: the saved.DAdjoint list of the first backward over ``sub``.
    Returns the saved.Hvp of the batched sweep (``n_head`` is the caller's to set)."""
    wait_pending(D)
    D._ensure_buffers()
    N, alpha = sub.NB, sub.alpha
    C = D.num_channels
    recs = sub.recs
    rec0 = recs[0]
    fr = rec0.blk.fromRGB
    H = rec0.H
    with _on_side(adj[0].gf, u):
        ops.fromrgb_wgrad(adj[0].gf, u, fr._gw, None, N, C, H, H, fr.c)
    cur = _bytes_first(lambda m, _: ops.fromrgb_fwd(u, fr.conv.weight.data, None, N, C, H, H, fr.c, 1.0, mask=m, mask_slope=fr.slope),
                       saved.Sign.inp(rec0), None, count=False)
    hvp = None
    t2 = None
    pn = bool(getattr(D, 'pixelnorm', False))
    injs = [saved.PNInjection() for _ in recs] if pn else None
    for idx, rec in enumerate(recs):
        blk, H = rec.blk, rec.H
        c1, c2 = blk.c1, blk.c2
        if rec.last:
            tmb, tstats = _mbstd_tangent(D, rec.inp, cur, rec.stats, c1.cin_store)
            hvp = saved.Hvp(tx=cur, tstats=tstats, gy_first=adj[idx].gmb, injs=injs)
            _wgrad(tmb, adj[idx].gz1, c1, N, H, bias=False, defer=True)
            t1 = _conv(tmb, c1, N, H, mask=saved.Sign.a1(rec), bias=False)
            if pn:
                t1, injs[idx].inj1 = ops.pixelnorm_tangent(t1, rec.a1, rec.r1, adj[idx].gy1)
            _wgrad(t1, adj[idx].gz2, c2, N, H, bias=False, defer=True)
            t2 = _conv(t1, c2, N, H, mask=saved.Sign.a2(rec), bias=False)
            if pn:
                t2, injs[idx].inj2 = ops.pixelnorm_tangent(t2, rec.a2, rec.r2, adj[idx].gy2)
        else:
            _wgrad(cur, adj[idx].gz1, c1, N, H, bias=False, defer=True)
            t1 = _conv(cur, c1, N, H, mask=saved.Sign.a1(rec), bias=False)
            if pn:
                t1, injs[idx].inj1 = ops.pixelnorm_tangent(t1, rec.a1, rec.r1, adj[idx].gy1)
            _wgrad(t1, adj[idx].gz2, c2, N, H, bias=False, defer=True)
            tpf = None
            if rec.first and alpha < 1.0:
                nfr = recs[idx + 1].blk.fromRGB
                with _on_side(adj[idx].gpf, u):
                    ops.fromrgb_wgrad(adj[idx].gpf, u, nfr._gw, None, N, C, H // 2, H // 2, nfr.c, pool=True)
                tpf = ops.fromrgb_fwd(u, nfr.conv.weight.data, None, N, C, H // 2, H // 2, nfr.c, 1.0,
                                      pool=True, mask=rec.pf, mask_slope=nfr.slope)
            pa, pb = (alpha, 1.0 - alpha) if tpf is not None else (1.0, 0.0)
            if pn:
                t2 = _conv(t1, c2, N, H, mask=saved.Sign.a2(rec), bias=False)
                t2, injs[idx].inj2 = ops.pixelnorm_tangent(t2, rec.a2, rec.r2, adj[idx].gy2)
                cur = ops.avgpool2_fwd(t2, tpf, pa, pb)
            else:                                                 # only the pooled tangent is needed downstream
                t2, cur = _conv_pool(t1, c2, N, H, bias=False, mask=saved.Sign.a2(rec), other=tpf, a=pa, b=pb, pool_only=True)
    # Linear: d/dw <ones, w . t2> = sum_n t2[n]
    ops.linear1_wgrad(_ones(N, u.device), t2, D._lin_gw, None)
    return hvp


def d_active_params(D, depth, alpha):
    """Parameters that take part at (depth, alpha) — the ones autograd would give a gradient."""
    nb = len(D.blocks)
    e = nb - 1 - depth
    layers = [D.blocks[e].fromRGB]
    if depth > 0 and alpha < 1.0:
        layers.append(D.blocks[e + 1].fromRGB)
    for j in range(e, nb):
        layers += [D.blocks[j].c1, D.blocks[j].c2]
    return layers


def d_exchange_layers(D, depth, alpha):
    """Everything that receives a gradient in a D step at (depth, alpha): the active conv / fromRGB layers + linear."""
    D._ensure_buffers()
    return d_active_params(D, depth, alpha) + [D._lin_layer]


def g_exchange_layers(G, depth, alpha):
    """Layers that receive a gradient in a G step at (depth, alpha) (the ``active`` list of generator_backward)."""
    G._ensure_buffers()
    return [lay for _, lay in G.stage_convs(depth)] + [t for t in G.rgb_heads(depth, alpha) if t is not None]


def discriminator_forward(D, x):
    """Plain ``D(x)`` (network.py:225-240): NCHW image batch -> scores [N,1]."""
    ops.require_gpu()
    x = _check_dev(x, 'D input')
    s, _ = d_forward(D, x, 1)
    return s.view(-1, 1)


# ------------------------------------------------------------------------------------------
# WGAN-GP steps
# ------------------------------------------------------------------------------------------
def _assign_grads(net, layers, linear=False):
    for m in layers:
        m.conv.weight.grad = m._gw
        m.conv.bias.grad = m._gb
    if linear:
        net.linear.weight.grad = net._lin_gw
        net.linear.bias.grad = net._lin_gb


# The real third on the second stream next to the generator's forward of the SAME step (3-image launches with nothing beside them), the
# fake third behind it on that stream, the mixed third on the main stream.  For every caller of wgan_gp_D_loss: the D step + gradient
# penalty alone 7.32 -> 7.21 ms at 1024^2, 9.58 -> 9.34 at 512^2, 16.63 -> 16.32 at 256^2.  The whole-batch forward stays the path of
# alpha < 1, a PixelNorm discriminator, the exact-global minibatch stddev, single-stream mode and the CPU emulation of the host tests.
REAL_THIRD_IN_STEP = True      # False: reference half of tests/test_e2e_gpu.py::test_three_pass_d_forward_matches_whole_batch_forward


class Objective(_collections.namedtuple('Objective', 'kind drift penalty weight target family augment', defaults=('pinned', None))):
    """What the loss block of a step computes: ``kind`` a key of ``ops.GAN_KINDS``, ``drift`` the weight of the
    s_r^2 term, ``penalty`` 'gp' | 'r1' | None with its ``weight`` (lambda / gamma) and, for 'gp', the ``target`` norm.  ``family`` names
    the kernels of the loss block: 'pinned' (csrc/gan_losses.hip, every rounding spelled out: what ``gan_losses`` builds) or 'original'
    (``pg_d_loss`` / ``pg_g_loss`` of csrc/elementwise.hip, contraction left to the compiler: WGAN-GP as ``wgan_gp_D_loss`` /
    ``wgan_gp_G_loss`` state it, kind 'wgan' with penalty 'gp' only).  The two are not bit-equal, so the family stays a property of the
    objective.  ``augment``: the ``augment.Augmenter`` every image D sees goes through (None: none, and not one launch differs), hashed
    by identity -- a plan bakes in the address of its accumulator.  Immutable and hashable: it is part of the key of a launch plan."""
    __slots__ = ()


WGAN_GP = Objective('wgan', 0.001, 'gp', 10.0, 1.0, 'original')      # the defaults of wgan_gp_D_loss


def _d_loss_block(obj, s, pen, N):
    if obj.family == 'original':
        return ops.d_loss(s, pen, N, obj.drift)                              # :48,55,62
    return ops.gan_d_loss(s, pen, N, obj.kind, obj.drift)


def _g_loss_block(obj, s):
    return ops.g_loss(s) if obj.family == 'original' else ops.gan_g_loss(s, obj.kind)


def _penalty_seed(obj, gimg, ss, N):
    if obj.penalty == 'r1':
        return ops.r1_seed(gimg, ss, obj.weight, 1.0 / N)
    return ops.gp_seed(gimg, ss, obj.weight, obj.target, 1.0 / N)        # :29-31


def _augmented(aug, x, table, out=None):
    """``x`` as D sees it under the Augmenter ``aug``: rows of ``table`` applied image by image (one launch on the current stream)."""
    return ops.augment_apply(x, table, aug.channel_mask, out=out)


def _step_table(objective, table, rows):
    """The parameter table of a step of ``objective``: None without an Augmenter, else ``table`` [rows, 8] int32 (a missing one is an error:
    the tables are drawn eagerly by the caller, wgan_gp_loss._d_loss / _g_loss, never inside a schedule)."""
    if objective.augment is None:
        if table is not None:
            raise ValueError('an augmentation table for an objective without an Augmenter')
        return None
    if table is None or tuple(table.shape) != (rows, ops.AUGMENT_COLS):
        raise ValueError('an objective with an Augmenter needs a table of %d rows (got %s)' % (rows, None if table is None else tuple(table.shape)))
    return table


def _count_real_signs(aug, s, N):
    """With a controller attached: the signs of the real scores into the Augmenter's accumulator, behind the loss block on this stream."""
    if aug is not None and aug.controller is not None:
        ops.score_signs(s[:N], aug.acc)


def d_loss_forward(D, G, real, latents, mix, objective, table=None):
    """Forward half of a D loss (wgan_gp_loss.py:36-65): three D passes batched as [real | fake | mixed], G without graph, and the first
    backward of the gradient penalty, with the loss block and the penalty seed of ``objective``.  R1 is the penalty at ``mix`` == 0, i.e.
    at the real images; an objective without a penalty takes one pass over [real | fake] (``_d_plain_loss_forward``; ``mix`` is not read).
    With ``objective.augment``: ``table`` [2N, 8] (reals, then fakes) -- the real third is the augmented real batch (in the place of the
    copy), the generator writes to a scratch tensor whose augmented form is the fake third; everything behind the two is untouched, so the
    penalty is taken at augmented images."""
    if objective.penalty is None:
        return _d_plain_loss_forward(D, G, real, latents, objective, table)
    ops.require_gpu()
    real = _check_dev(real, 'real images')
    latents = _check_dev(latents, 'latents')
    mix = _check_dev(mix, 'mixing factors').view(-1)
    N = real.shape[0]
    aug, table = objective.augment, _step_table(objective, table, 2 * real.shape[0])
    D._sync_version()
    fake_done = None
    arena_st = None
    if (REAL_THIRD_IN_STEP and float(D.alpha) >= 1.0 and not getattr(D, 'pixelnorm', False) and ASYNC_WGRAD and real.is_cuda
            and hasattr(ops, 'Arena') and D._rt.global_stddev is None     # (exact-global stddev: its collectives stay on one stream, one pass; host tests run the schedules on a CPU emulation of ops: one pass there)
            and _three_pass_buffers(D, real) is not None):
        # the three thirds as three passes into one set of batched tensors (see REAL_THIRD_IN_STEP)
        st = arena_st = D._rt.d_fwd_buffers
        x3 = st.x3
        main = torch.cuda.current_stream(torch._C._cuda_getDevice())
        side = _side_stream()
        wait_pending(D)                                                       # on the MAIN stream, before the fork: the side pass's own wait_pending would consume the event there and leave the mixed third un-ordered
        step_start = torch.cuda.Event()
        _record_event(step_start, main)                                       # (everything the previous step left on the main stream)
        probe('D.start')
        if aug is None:
            d_step_generator(D, G, latents, x3[N:2 * N])                    # :51-52  -- issued first: the host feeds the critical path before the side work
        else:                                                                 # (G(z) into the buffers' scratch, its augmented form into the fake third: on the generator's stream, ahead of the edges that release it)
            if st.g_out is None:
                st.g_out = torch.empty_like(x3[:N])
            d_step_generator(D, G, latents, st.g_out)
            _augmented(aug, st.g_out, table[N:], out=x3[N:2 * N])
        probe('D.g_fwd_end')
        with torch.cuda.stream(side):
            _wait_event(side, step_start)
            probe('D.side_start')
            if aug is None:
                ops.axpby_mask(real, a=1.0, out=x3[:N])                       # (the copy into the batched image buffer too, so that the generator starts at once: -0.03 ms)
            else:
                _augmented(aug, real, table[:N], out=x3[:N])                  # (in the copy's place)
            real_copied = torch.cuda.Event()
            _record_event(real_copied, side)
            with st.arena.pass_(0):
                s_r, ctx_r = d_forward(D, x3[:N], groups=1)                   # :47
            probe('D.real_end')
        real.record_stream(side)
        if aug is not None:
            table.record_stream(side)                                         # (read by the real third's gather on that stream)
        _wait_stream(side, main)
        with torch.cuda.stream(side):
            probe('D.fake_start')
            with st.arena.pass_(2):
                s_f, ctx_f = d_forward(D, x3[N:2 * N], groups=1)              # :54
            fake_done = torch.cuda.Event()
            _record_event(fake_done, side)
            probe('D.fake_end')
        _early_g_on_side(D, main, side)
        _wait_event(main, real_copied)
        ops.gp_mix(x3[:N], x3[N:2 * N], mix, out=x3[2 * N:])                  # :19
        probe('D.mix_end')
        with st.arena.pass_(3):
            s_m, ctx_m = d_forward(D, x3[2 * N:], groups=1)                   # :20
        probe('D.mixed_fwd_end')
        ctx = saved.DContext.merge([ctx_r, ctx_f, ctx_m])
        s = s_r._base if s_r._base is not None else s_r
    else:
        x3 = torch.empty((3 * N,) + tuple(real.shape[1:]), device=real.device, dtype=torch.float32)
        if aug is None:
            ops.axpby_mask(real, a=1.0, out=x3[:N])                           # device copy (plumbing; a C-ABI launch so that plans.py records it)
            d_step_generator(D, G, latents, x3[N:2 * N])                    # :51-52  (no graph kept)
        else:
            _augmented(aug, real, table[:N], out=x3[:N])
            _augmented(aug, d_step_generator(D, G, latents, torch.empty_like(real)), table[N:], out=x3[N:2 * N])
        ops.gp_mix(x3[:N], x3[N:2 * N], mix, out=x3[2 * N:])                  # :19
        s, ctx = d_forward(D, x3, groups=3)                                   # :47,54,20
    sub = ctx.slice(2 * N, 3 * N, 2, 3)
    gimg, adj = d_backward(D, sub, _ones(N, real.device), full=False, want_gimg=True, save_adjoints=True)  # :25-28
    ss = ops.row_sumsq(gimg)
    gp, u = _penalty_seed(objective, gimg, ss, N)
    probe('D.gp_bwd_end')
    if fake_done is not None:
        _wait_event(torch.cuda.current_stream(torch._C._cuda_getDevice()), fake_done)
    d_cost, d_real_loss, d_fake_loss, gscore = _d_loss_block(objective, s, gp, N)
    _count_real_signs(aug, s, N)
    probe('D.loss_end')
    state = saved.DLossState(D=D, ctx=ctx, sub=sub, adj=adj, u=u, gscore=gscore, N=N, scores=s, gp=gp)
    if arena_st is not None:
        state.arena_use, state.arena_st = _ArenaUse(), arena_st
        arena_st.owner = _weakref.ref(state.arena_use)
    return d_cost, d_real_loss, d_fake_loss, state


def _three_pass_buffers(D, real):
    """The per-(network, stage, shape) arena of the three-pass forward, or None when the activations of an earlier D loss of this
    network still live in it (that loss is alive and has not been back-propagated): the caller then takes the allocating one-pass form."""
    key = (int(D.depth), tuple(real.shape))
    st = D._rt.d_fwd_buffers
    if st is None or st.key != key:
        st = D._rt.d_fwd_buffers = _DForwardBuffers()
        st.key = key
        st.x3 = torch.empty((3 * real.shape[0],) + tuple(real.shape[1:]), device=real.device, dtype=torch.float32)
        return st
    return st if _arena_free(st) else None


# ---- the G step's generator forward, ahead of time -------------------------------------------------------------------------------------
# The un-traced phase timeline of the 1024^2 step (tools/phase_timeline.py, round 6) shows the main stream busy from the first launch to the
# last -- it IS the critical path -- while the second stream idles under the gradient penalty's first backward and the tangent pass (1.6 ms
# of 3-image launches: the weight gradients of the tangent pass ride in the sweep's launches) and again under the whole first half of the G
# step.  The G step opens with G(z') on fresh latents (trainer.py:103-105) with the SAME generator weights the D step used (G is updated at the
# end of the G step only), so that pass does not have to wait for anything the D step computes: Trainer hands the latents to the D step
# (``request_early_g``), the D step enqueues G(z') -- with its activations kept for the backward -- on the second stream behind the fake
# third, and the G step starts from the finished pass with D's forward.  Same kernels, same inputs, same results.
# Same-box pairs, ms per step off | on (round 6): 1024^2 10.344 | 10.263, 10.358 | 10.242, 10.363 | 10.219; 512^2 13.52 | 13.39, 13.53 | 13.37;
# 256^2 23.04 | 22.83; 64^2 (minibatch 16: the chip is full) 14.54 | 14.66; 16^2 5.25 | 5.34 -- on from 256^2 up (the stages whose minibatch
# leaves the chip partly idle).
EARLY_G_FORWARD = True         # False: reference half of tests/test_e2e_gpu.py::test_trainer_early_g_forward_matches_in_step_forward
EARLY_G_MIN_RES = 256          # 4 in tests/test_e2e_gpu.py::test_early_g_forward_is_the_same_pass (the pass at a small test stage)
# Two forms: 'side' = on the second stream behind the fake third (the stages whose minibatch leaves the chip partly idle: from 256^2 up);
# 'batched' = ONE generator pass over [z | z'] in place of the D step's G(z) (the launch-bound 4x4 stage: half the generator launches per
# iteration, 1.166 -> 0.997 ms per step).  Same-box pairs, ms per step side | batched: 1024^2 10.31 | 10.55, 10.28 | 10.48, 10.33 | 10.46 (a
# 6-image pass takes 1.50 ms against 1.02 and holds the fake third back); 512^2 13.40 | 13.51; 256^2 23.25 | 23.29; off | batched: 128^2
# 20.05 | 20.23, 64^2 14.66 | 14.77, 16^2 5.24 | 5.42.
EARLY_G_MODE = 'auto'          # 'side' / 'batched' in the two tests above: one form wherever the pass runs at all
_EARLY_G_BATCHED_MAX_RES = 4


def early_g_mode(depth):
    """'side' | 'batched' | None (the G step runs its own generator pass) for a growth stage."""
    if not EARLY_G_FORWARD:
        return None
    res = 4 * 2 ** int(depth)
    if EARLY_G_MODE == 'auto':
        return 'batched' if res <= _EARLY_G_BATCHED_MAX_RES else 'side' if res >= EARLY_G_MIN_RES else None
    return EARLY_G_MODE if (res >= EARLY_G_MIN_RES or res <= _EARLY_G_BATCHED_MAX_RES) else None
EARLY_G_STATS = {'passes': 0, 'used': 0, 'dropped': 0}


class EarlyG(object):
    """A finished (enqueued) ``generator_forward(G, latents, save=True)``: output image, context, the latents tensor it was computed from
    (identity: what the G loss will be handed), what it was computed with, and the event that closes it on the second stream."""
    __slots__ = ('fake', 'ctx', 'latents', 'stamp', 'event')


def d_step_generator(D, G, latents, out):
    """The D step's generator pass G(z) -> ``out`` (wgan_gp_loss.py:51-52, no graph kept).  EARLY_G_MODE 'batched': when Trainer has
    announced the G step's latents z' (``request_early_g``) the two passes run as ONE pass over [z | z'] -- the same weights, twice the
    images per launch, and the <= 64x64 layers of a 3-image pass are latency-bound launches that take 6 images in nearly the same time --
    and the second half (with its activations) is left for the G step as an ``EarlyG``."""
    req = D._rt.early_g_request if early_g_mode(G.depth) == 'batched' else None
    if req is None or req[0] is not G or tuple(req[1].shape) != tuple(latents.shape):
        return generator_forward(G, latents, out=out)
    D._rt.early_g_request = None
    zg = _check_dev(req[1], 'latents')
    N = latents.shape[0]
    z2 = torch.empty((2 * N,) + tuple(latents.shape[1:]), device=latents.device, dtype=torch.float32)
    ops.axpby_mask(latents, a=1.0, out=z2[:N])
    ops.axpby_mask(zg, a=1.0, out=z2[N:])
    eg = EarlyG()
    eg.fake = torch.empty_like(out)
    (img, _), ctx = generator_forward(G, z2, save=True, pair_out=(out, eg.fake))
    eg.ctx = ctx.slice(N, 2 * N)
    eg.event = torch.cuda.Event()
    _record_event(eg.event, torch.cuda.current_stream(torch._C._cuda_getDevice()))
    eg.latents = zg
    eg.stamp = (G._param_version, int(G.depth), float(G.alpha))
    G._rt.early_fwd = eg
    EARLY_G_STATS['passes'] += 1
    return img


def request_early_g(D, G, latents):
    """Trainer, before the D loss: the next G loss of this iteration will be ``wgan_gp_G_loss(G, D, latents)``."""
    D._rt.early_g_request = (G, latents)


def _early_g_on_side(D, main, side):
    """Inside ``d_loss_forward``, right after the fake third was queued on the second stream: the requested generator pass behind it."""
    req = D._rt.take('early_g_request')
    if req is None or early_g_mode(req[0].depth) != 'side':
        return
    G, z = req
    z = _check_dev(z, 'latents')
    with torch.cuda.stream(side):
        probe('D.early_g_start')
        eg = EarlyG()
        eg.fake, eg.ctx = generator_forward(G, z, save=True)
        eg.event = torch.cuda.Event()
        _record_event(eg.event, side)
        probe('D.early_g_end')
    # allocated under the second stream's context, consumed (and eventually freed) on the main stream
    eg.fake.record_stream(main)
    for t in saved.tensors(eg.ctx):
        t.record_stream(main)
    eg.latents = z
    eg.stamp = (G._param_version, int(G.depth), float(G.alpha))
    G._rt.early_fwd = eg
    EARLY_G_STATS['passes'] += 1


def take_early_g(G, latents):
    """The generator pass the D step left for exactly these latents, if it is still valid (same tensor, same weights, same stage); the
    current stream is ordered behind it.  None: the caller runs the pass itself."""
    eg = G._rt.take('early_fwd')
    if eg is None:
        return None
    if eg.latents is not latents or eg.stamp != (G._param_version, int(G.depth), float(G.alpha)):
        EARLY_G_STATS['dropped'] += 1
        return None
    _wait_event(torch.cuda.current_stream(torch._C._cuda_getDevice()), eg.event)
    EARLY_G_STATS['used'] += 1
    return eg


def _backward(net, scale, sweep, probes, linear=False, may_skip_join=False):
    """What ``backward()`` of every loss does around its ``sweep()`` (which returns the layers that received a gradient): the flat gradient
    zeroed, nothing travelling early and nothing pending before it; behind it the deferred contributions flushed, the weight-gradient stream
    joined, the gradients rescaled and assigned.  ``probes``: the tags of the sweep's end on the main and on the second stream."""
    net._ensure_buffers()
    ops.zero_(net._flat_grad)
    if scale != 1.0:
        net._rt.grad_hook = None                 # the gradients are rescaled after the sweep: nothing may travel early
    live = _live_conv_layers(net)
    for lay in live:                             # (nothing of an aborted earlier step may ride along)
        lay._pending_wgrad = None
    active = sweep()
    for lay in live:                             # (a deferred tangent contribution that no launch of the sweep carried)
        _flush_wgrad(lay)
    probe(probes[0])
    if PROBES is not None and ASYNC_WGRAD and net._flat_param.is_cuda:
        with torch.cuda.stream(_side_stream()):
            probe(probes[1])
    if not (may_skip_join and net._rt.skip_join and scale == 1.0):
        _join_side()         # default: the gradients are complete for whatever the caller does next on this stream
    # (Trainer sets skip_join when the whole D update follows on the second stream, in order behind the weight
    #  gradients: the main stream then goes straight on to the G step instead of idling under the last, largest
    #  weight-gradient launches of the 1024^2 layers)
    if scale != 1.0:
        ops.axpby_mask(net._flat_grad, a=scale, out=net._flat_grad)
    _assign_grads(net, active, linear=linear)
    return active


def d_loss_backward(state, scale=1.0):
    """``D_cost.backward()`` (trainer.py:98): tangent pass + batched [real|fake|mixed] adjoint sweep; for a state without a penalty
    (``_d_plain_loss_forward``: no ``sub`` / ``adj`` / ``u``) the adjoint sweep over [real | fake] alone."""
    D, ctx, N = state.D, state.ctx, state.N
    tok = state.arena_use
    if tok is not None:
        if state.arena_st.owner() is not tok:     # (second line of defence: a retained loss back-propagated again after a later forward)
            raise RuntimeError('the activations of this D loss were overwritten by a later D-loss forward on the same network')
        tok.consumed = True

    def sweep():
        if state.sub is None:
            d_backward(D, ctx, state.gscore, full=True, want_gimg=False)
        else:
            hvp = d_tangent_wgrad(D, state.sub, state.adj, state.u)
            probe('D.tangent_end')
            hvp.n_head = 2 * N                   # [real | fake] take the score gradients, the mixed third the injections only
            d_backward(D, ctx, state.gscore[:2 * N], full=True, want_gimg=False, hvp=hvp)
        return d_active_params(D, ctx.depth, ctx.alpha)
    _backward(D, scale, sweep, ('D.sweep_end', 'D.wgrad_end'), linear=True, may_skip_join=True)


def _d_plain_loss_forward(D, G, real, latents, objective, table=None):
    """The D step of an objective without a penalty: ONE whole-batch pass over [real | fake], then the loss block.  No mixed third, no
    first backward, no tangent pass.  ``table``: as in ``d_loss_forward``."""
    ops.require_gpu()
    real = _check_dev(real, 'real images')
    latents = _check_dev(latents, 'latents')
    N = real.shape[0]
    aug, table = objective.augment, _step_table(objective, table, 2 * real.shape[0])
    D._sync_version()
    x2 = torch.empty((2 * N,) + tuple(real.shape[1:]), device=real.device, dtype=torch.float32)
    if aug is None:
        ops.axpby_mask(real, a=1.0, out=x2[:N])
        d_step_generator(D, G, latents, x2[N:])
    else:
        _augmented(aug, real, table[:N], out=x2[:N])
        _augmented(aug, d_step_generator(D, G, latents, torch.empty_like(real)), table[N:], out=x2[N:])
    s, ctx = d_forward(D, x2, groups=2)
    d_cost, d_real_loss, d_fake_loss, gscore = _d_loss_block(objective, s, None, N)
    _count_real_signs(aug, s, N)
    return d_cost, d_real_loss, d_fake_loss, saved.DLossState(D=D, ctx=ctx, gscore=gscore, N=N, scores=s)


def g_loss_forward(G, D, latents, objective, table=None):
    """wgan_gp_G_loss (wgan_gp_loss.py:68-74) with the generator term of ``objective`` (-s for the 'wgan' kind).  With
    ``objective.augment``: D scores the fakes augmented by ``table`` [N, 8], which the state keeps for the transpose in the backward."""
    ops.require_gpu()
    latents = _check_dev(latents, 'latents')
    table = _step_table(objective, table, latents.shape[0])
    D._sync_version()
    G._sync_version()
    probe('G.start')
    eg = take_early_g(G, latents)
    if eg is not None:
        fake, gctx = eg.fake, eg.ctx
    else:
        fake, gctx = generator_forward(G, latents, save=True)
    probe('G.g_fwd_end')
    if table is not None:
        fake = _augmented(objective.augment, fake, table)
    s, dctx = d_forward(D, fake, 1, keep_input=False)
    g_cost, gscore = _g_loss_block(objective, s)
    probe('G.d_fwd_end')
    return g_cost, saved.GLossState(G=G, D=D, gctx=gctx, dctx=dctx, gscore=gscore, table=table)


def g_loss_backward(state, scale=1.0):
    """``G_cost.backward()`` (trainer.py:111).  D's weight gradients, which the reference computes here
    and throws away at its next D.zero_grad(), are not computed."""
    G, D = state.G, state.D

    def sweep():
        gimg, _ = d_backward(D, state.dctx, state.gscore, full=False, want_gimg=True)
        if state.table is not None:
            gimg = ops.augment_adjoint(gimg, state.table)     # back through the augmentation: the same table, the exact transpose
        probe('G.d_bwd_end')
        return generator_backward(G, state.gctx, gimg)
    state.active_g = _backward(G, scale, sweep, ('G.g_bwd_end', 'G.wgrad_end'))
