"""Smoothed generator ``Gs``: an exponential running average of G's weights, kept on the device (Karras et al. 2018, "Training
configuration": every sample grid, inference snapshot and sliced-Wasserstein figure of the paper comes from Gs, decay 0.999; the reference
has none).  G's Adam(beta1 = 0) update is sign-like and G oscillates from step to step; the average takes that out.

``GeneratorEMA`` owns Gs, a ``Generator`` of G's configuration and flat layout, and moves it once per G update with ONE ``pg_ema_f32``
launch over the whole flat parameter buffer (padding, not-yet-grown blocks and retired toRGB layers included: the TF implementation's
semantics -- a toRGB that stopped training keeps converging to its final value, and there is no per-run launch logic).  Opt-in:
``Trainer(..., g_ema=GeneratorEMA(G))``; the output plugins then read ``trainer.g_ema.network()``."""
import copy

import torch

from . import engine, ops, runtime

DEFAULT_BETA = 0.999


def _layout(net):
    flat = getattr(net, '_flat_param', None)
    if flat is None:
        raise ValueError('GeneratorEMA needs a Generator of this package (one flat parameter buffer); got %s' % type(net).__name__)
    return list(net._flat_offsets), flat.numel()


class GeneratorEMA(object):
    """``GeneratorEMA(G, beta=0.999, halflife_kimg=None, Gs=None)``.

    ``beta``: decay per update.  ``halflife_kimg``: the decay follows the images of each iteration instead,
    ``beta = 0.5 ** (nimg / (halflife_kimg * 1000))``, which keeps the horizon fixed in images while the minibatch goes 16 -> 3 across
    the stages; giving both raises ``ValueError``.  ``Gs``: a smoothed generator to go on from (``plugins.load_smoothed_generator``);
    by default the average starts as a copy of G.  Gs never gets gradients or Adam state."""

    def __init__(self, G, beta=DEFAULT_BETA, halflife_kimg=None, Gs=None):
        if halflife_kimg is not None and beta != DEFAULT_BETA:
            raise ValueError('give beta or halflife_kimg, not both')
        if not 0.0 <= float(beta) <= 1.0:                   # (False for a NaN too)
            raise ValueError('beta must be in [0, 1], got %r' % (beta,))
        if halflife_kimg is not None and not float(halflife_kimg) > 0.0:
            raise ValueError('halflife_kimg must be positive, got %r' % (halflife_kimg,))
        self.beta = float(beta)
        self.halflife_kimg = None if halflife_kimg is None else float(halflife_kimg)
        want = _layout(G)
        fresh = Gs is None
        if fresh:
            Gs = copy.deepcopy(G)                           # (through Generator.__getstate__ / __setstate__: no gradient buffers, a run-time object of its own)
        elif _layout(Gs) != want:
            raise ValueError('Gs does not have the flat parameter layout of G (%d against %d elements): another configuration'
                             % (_layout(Gs)[1], want[1]))
        Gs.to(G._flat_param.device)                         # (re-flattens: its parameters are views of ONE buffer of its own, on G's device)
        if _layout(Gs) != want:
            raise ValueError('the copy of G does not have its flat parameter layout')
        for p in Gs.parameters():
            p.requires_grad_(False)
        if fresh:
            with torch.no_grad():
                Gs._flat_param.copy_(G._flat_param)
            Gs.mark_params_changed()
        self.G, self.Gs = G, Gs

    def decay(self, nimg):
        """beta of an iteration that showed ``nimg`` images (all ranks)."""
        if self.halflife_kimg is None:
            return self.beta
        return 0.5 ** (nimg / (self.halflife_kimg * 1000.0))

    def await_last(self):
        """The current stream waits for the last launch of ``update`` (no-op when that ran inline).  The event stays: it has two waiters."""
        ev = runtime.of(self.G).ema_ev
        if ev is not None:
            torch.cuda.current_stream(torch._C._cuda_getDevice()).wait_event(ev)

    @torch.no_grad()
    def update(self, nimg):
        """Gs += (1 - beta) * (G - Gs) over the whole flat buffer; call after G's optimizer step.  With two streams the launch goes on the
        engine's second stream (2.4 ms of slack per 1024x1024 step; the main stream is the critical path) behind everything
        queued so far on the current one -- Adam(G) above all -- and leaves ``G._rt.ema_ev`` for the next writer of G's parameters and for
        ``network()``.  Gs's derived weights are refreshed by its next forward pass, not here."""
        G, Gs = self.G, self.Gs
        src = G._flat_param                                 # read on every call: a re-flatten of G (.cuda(), .float()) replaces the buffer
        if Gs._flat_param.device != src.device or Gs._flat_param.dtype != src.dtype:
            self.await_last()                               # (G moved: Gs follows, behind the last launch into its old buffer)
            Gs.to(device=src.device, dtype=src.dtype)
        dst = Gs._flat_param
        if dst.numel() != src.numel():
            raise ValueError('G was rebuilt: %d parameters against %d averaged ones' % (src.numel(), dst.numel()))
        beta = self.decay(nimg)
        rt = runtime.of(G)
        cur = torch.cuda.current_stream(torch._C._cuda_getDevice()) if src.is_cuda else None
        side = engine._side_stream() if (cur is not None and engine.ASYNC_WGRAD) else None
        if side is None or side == cur or torch.cuda.is_current_stream_capturing():
            self.await_last()                               # (a change of mode between two calls: behind an earlier second-stream launch)
            ops.ema(dst, src, beta)                         # single-stream mode, host tensors: inline
            rt.ema_ev = None
        else:
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                ops.ema(dst, src, beta)
                ev = torch.cuda.Event()
                ev.record(side)
            for buf in (dst, src):                          # used on the second stream: the allocator must not hand the block on before that
                buf.record_stream(side)
            rt.ema_ev = ev
        Gs.mark_params_changed()

    def network(self):
        """Gs at G's growth stage (the DepthManager drives ``trainer.G`` / ``trainer.D`` only), readable on the current stream."""
        self.Gs.depth, self.Gs.alpha = self.G.depth, self.G.alpha
        self.await_last()
        return self.Gs
