"""Latent projection: the latent whose generated image matches a given one (DESIGN.md §7 "Latent projection").

Everything else that looks at a trained generator runs ``z -> G(z)``; this runs the other way.  ``Projector(net).project(targets)``
minimises, per target, the pyramid loss of ``ops.pyramid_loss`` (include/pggan_hip_projection.h: squared error of the box-mean pyramid
of ``G(z) - target``, sides r .. 4) over z with Adam on a cosine learning-rate schedule, entirely on the device and without a host
synchronisation inside the loop.  It works for 1-, 2-, 3- and 4-channel networks alike.

One step is
  1. ``engine.generator_forward(net, z, save=True)``: the image and the saved activations (outside ``ops.Arena`` every saved tensor is
     an allocation of its own and outlives the call at every stage); the latent PixelNorm's factor, which the forward pass does not
     keep, comes from the projector's own ``ops.pixelnorm_fwd``;
  2. ``ops.pyramid_loss``: per-sample loss and image gradient;
  3. the frozen-weight input-gradient sweep, plain ``ops`` calls only: toRGB's backward-data (and the fade-in branch's, added behind
     the top block), per block the adjoint of (LeakyReLU -> PixelNorm) and the backward-data conv of c2 (one launch,
     ``ops.conv2d_pnbwd``), the backward-data conv of c1 and ``ops.upsample2_bwd``; in block 0 c1's backward-data conv is the 4x4 kernel
     with pad 4 - 1 - 3 = 0 on the 4x4 map, which gives [N,1,1,latent], and the latent PixelNorm's adjoint closes the sweep.  No weight
     gradient is computed and nothing is written to the network's gradient buffer;
  4. ``ops.adam`` on the flat latents with the projector's own moments.

The sweep stays out of the engine's run-time state on purpose.  ``engine._wt`` / ``engine._wino(transposed=True)`` mark layers and the
network (``_wt_wanted``, ``bwd_wanted``), invalidate ``derived_ver`` and take part in the cross-stream events of the training step; an
evaluation copy that has never run a backward pass would start to pay for backward-data copies at every later update.  The projector
therefore owns its flipped / transposed weight copies (``ops.pack_dgrad_weights`` into a buffer of its own, refreshed when the flat
buffer's address, ``net._param_version`` or the depth has moved, the way ``sampling.Sampler`` owns its bf16 twin), refers to the network
weakly and sets nothing on it, its layers or ``net._rt``.  The forward pass is the network's own and does what ``net.forward`` does.

The small-map backward-data convs commit K slices with atomics, so dz is not bit-reproducible (the loss and its image gradient are)."""
import collections
import math
import weakref

import torch

from . import engine, ops

Projection = collections.namedtuple('Projection', 'z images loss history')


class Projector(object):
    """``Projector(net, steps=200, lr=0.1, betas=(0.9, 0.999), level_weights=None, seed=0)``: projection onto the images of a
    ``Generator`` (``G`` or ``GeneratorEMA.network()``) at ``net.depth`` / ``net.alpha`` as they are at the call.

    ``project(targets, z0=None)``: fp32 device tensor [N,C,r,r] -> ``Projection(z [N,latent], images [N,C,r,r], loss [N], history
    [steps,N])``: the latents after the last step (not a best-of), their images and losses, and the loss before every step, all device
    tensors.  The start latents are ``z0`` or draws of ``utils.device_latents`` with ``seed``.  The learning rate of step t = 0 ..
    steps - 1 is ``lr (1 + cos(pi t / steps)) / 2``; the bias corrections are computed on the host per step, as ``FusedAdam`` does.
    ``loss_and_grad(z, targets)`` -> ``(loss [N], dz [N,latent])``: one forward pass, loss and sweep.
    ``level_weights``: weights of the pyramid levels from the finest, as in ``ops.pyramid_loss``.
    Raises ``ValueError`` at construction for a network this sweep does not take, naming the layer."""

    def __init__(self, net, steps=200, lr=0.1, betas=(0.9, 0.999), level_weights=None, seed=0, eps=1e-8):
        if getattr(net, '_flat_param', None) is None or not hasattr(net, 'block0') or not hasattr(net, 'blocks'):
            raise ValueError('Projector needs a Generator of this package (one flat parameter buffer); got %s' % type(net).__name__)
        if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
            raise ValueError('Projector: steps must be a positive integer, got %r' % (steps,))
        if not float(lr) > 0.0 or not math.isfinite(float(lr)):
            raise ValueError('Projector: lr must be a positive number, got %r' % (lr,))
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError('Projector: betas must be two numbers in [0, 1), got %r' % (betas,))
        if not float(eps) > 0.0:
            raise ValueError('Projector: eps must be positive, got %r' % (eps,))
        if not 1 <= int(net.num_channels) <= ops.PYR_MAX_C:
            raise ValueError('Projector: %d image channels (1 .. %d)' % (net.num_channels, ops.PYR_MAX_C))
        if int(net.latent_size) % 4:
            raise ValueError('Projector: latent size %d is not a multiple of 4' % net.latent_size)
        for name, lay in net.stage_convs(len(net.blocks)):
            first = name == 'block0.c1'
            if (lay.ksize, lay.pad) != ((4, 3) if first else (3, 1)):
                raise ValueError('Projector: layer %s is %dx%d pad %d, not the %s conv the sweep is written for'
                                 % (name, lay.ksize, lay.ksize, lay.pad, '4x4 pad-3' if first else '3x3 pad-1'))
            if lay.act is None:
                raise ValueError('Projector: layer %s has no activation; the sweep reads LeakyReLU / ReLU branches from the saved outputs' % name)
        if level_weights is not None:
            level_weights = [float(w) for w in level_weights]
            top = ops.pyramid_levels(4 * 2 ** len(net.blocks))
            if not 1 <= len(level_weights) <= top or any(not (0.0 <= w < float('inf')) for w in level_weights):
                raise ValueError('Projector: level_weights must be 1 .. %d finite non-negative numbers, got %r' % (top, level_weights))
        self._net = weakref.ref(net)
        self.steps, self.lr, self.betas, self.eps = int(steps), float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.level_weights, self.seed = level_weights, int(seed)
        self._wt_buf = None              # the flipped / transposed copies of the live layers' weights, one after the other
        self._wt = {}                    # id(layer) -> its view [ks, ks, cin_store, cout] of the buffer
        self._seen = None                # (address of the flat buffer, net._param_version, depth) of the last pack
        self._scratch = None             # fp64 scratch of ops.pyramid_loss

    def network(self):
        net = self._net()
        if net is None:
            raise RuntimeError('the network of this Projector is gone')
        return net

    # ------------------------------------------------------------------------------------------ weights
    def _refresh(self, net, depth):
        flat = net._flat_param
        key = (flat.data_ptr(), net._param_version, depth)
        if self._seen == key:
            return
        layers = net.stage_convs(depth)
        total = sum(lay.conv.weight.numel() for _, lay in layers)
        if self._wt_buf is None or self._wt_buf.device != flat.device or self._wt_buf.numel() != total:
            self._wt_buf = torch.empty(total, device=flat.device, dtype=torch.float32)
        self._wt, off = {}, 0
        for _, lay in layers:
            w = lay.conv.weight.data
            ks, _, co, ci = w.shape
            view = self._wt_buf[off:off + w.numel()].view(ks, ks, ci, co)
            ops.pack_dgrad_weights(w, view)
            self._wt[id(lay)] = view
            off += w.numel()
        self._seen = key

    def packed_weights(self):
        """The projector's backward-data weight copies as they are (a flat fp32 device tensor; None before the first pass)."""
        return self._wt_buf

    # ------------------------------------------------------------------------------------------ one pass
    def _levels(self, r):
        if self.level_weights is None:
            return None
        if len(self.level_weights) > ops.pyramid_levels(r):
            raise ValueError('Projector: %d level weights for %dx%d images (%d levels)'
                             % (len(self.level_weights), r, r, ops.pyramid_levels(r)))
        return self.level_weights

    def _check(self, net, z, targets):
        z = engine._check_dev(z, 'latents')
        targets = engine._check_dev(targets, 'targets')
        r = 4 * 2 ** int(net.depth)
        if z.dim() != 2 or z.shape[1] != net.latent_size:
            raise ValueError('latents %s (expected [N, %d])' % (tuple(z.shape), net.latent_size))
        if tuple(targets.shape) != (z.shape[0], int(net.num_channels), r, r):
            raise ValueError('targets %s (expected %s at depth %d)' % (tuple(targets.shape), (z.shape[0], int(net.num_channels), r, r), int(net.depth)))
        return z, targets

    def _pyramid(self, img, targets, want_grad):
        words = ops.pyramid_scratch_words(*img.shape[:3])
        if self._scratch is None or self._scratch.device != img.device or self._scratch.numel() < words:
            self._scratch = torch.empty(words, device=img.device, dtype=torch.float64)
        return ops.pyramid_loss(img, targets, self._levels(img.shape[-1]), want_grad=want_grad, scratch=self._scratch)

    def _sweep(self, net, ctx, g, rz):
        """Image gradient g [N,C,r,r] -> dz [N,latent] on the linear piece the forward pass ``ctx`` selected."""
        N, depth, alpha = ctx.N, ctx.depth, ctx.alpha
        C = int(net.num_channels)
        b0 = net.block0
        extra = None
        t, pt = net.rgb_heads(depth, alpha)
        if depth == 0:
            gh = ops.torgb_bwd_data(g, t.conv.weight.data, N, C, 4, 4, t.c)
        else:
            H = ctx.recs[-1].H
            gh = ops.torgb_bwd_data(g, t.conv.weight.data, N, C, H, H, alpha * t.c)
            if pt is not None:
                extra = ops.torgb_bwd_data(g, pt.conv.weight.data, N, C, H // 2, H // 2, (1.0 - alpha) * pt.c, down=True)
        for rec in reversed(ctx.recs):
            c1, c2, H = rec.blk.c1, rec.blk.c2, rec.H
            gz2 = ops.pixelnorm_lrelu_bwd(gh, rec.a2, rec.r2, c2.slope, inplace=True)
            # backward-data conv of c2 + the adjoint of c1's (LeakyReLU -> PixelNorm)
            gz1 = ops.conv2d_pnbwd(gz2, self._wt[id(c2)], rec.a1, rec.r1, N, H, H, 3, 1, c2.c, c1.slope)
            gu = ops.conv2d(gz1, self._wt[id(c1)], None, N, H, H, 3, 1, c1.c, 1.0)
            gh = ops.upsample2_bwd(gu)
            if gh.shape[-1] != c1.ch_in:                   # (zero-padded stored input channels carry no gradient)
                gh = gh[..., :c1.ch_in].contiguous()
            if extra is not None:                          # the fade-in branch joins behind the top block
                gh = ops.axpby_mask(gh, other=extra, a=1.0, b=1.0, out=gh)
                extra = None
        gz2 = ops.pixelnorm_lrelu_bwd(gh, ctx.y2, ctx.r2, b0.c2.slope, inplace=True)
        gz1 = ops.conv2d_pnbwd(gz2, self._wt[id(b0.c2)], ctx.y1, ctx.r1, N, 4, 4, 3, 1, b0.c2.c, b0.c1.slope)
        gzn = ops.conv2d(gz1, self._wt[id(b0.c1)], None, N, 4, 4, 4, 0, b0.c1.c, 1.0)         # [N,1,1,cin_store]
        gzn = gzn.view(N, -1)
        if gzn.shape[1] != net.latent_size:
            gzn = gzn[:, :net.latent_size].contiguous()
        if net.normalize_latents:
            gzn = ops.pixelnorm_lrelu_bwd(gzn, ctx.zn, rz, 1.0, inplace=True)
        return gzn

    def _forward(self, net, z):
        img, ctx = engine.generator_forward(net, z, save=True)
        rz = ops.pixelnorm_fwd(z, net.eps)[1] if net.normalize_latents else None
        self._refresh(net, ctx.depth)
        return img, ctx, rz

    def loss_and_grad(self, z, targets, return_context=False):
        """``(loss [N], dz [N,latent])`` of the latents ``z`` against ``targets``; ``return_context``: also the image and the forward
        pass's saved activations (``saved.GContext``), whose signs say on which linear piece dz was taken."""
        net = self.network()
        z, targets = self._check(net, z, targets)
        img, ctx, rz = self._forward(net, z)
        loss, g = self._pyramid(img, targets, True)
        dz = self._sweep(net, ctx, g, rz)
        return (loss, dz, img, ctx) if return_context else (loss, dz)

    # ------------------------------------------------------------------------------------------ the search
    def learning_rate(self, t):
        return self.lr * 0.5 * (1.0 + math.cos(math.pi * t / self.steps))

    def project(self, targets, z0=None):
        net = self.network()
        targets = engine._check_dev(targets, 'targets')
        if targets.dim() != 4 or targets.shape[0] < 1:
            raise ValueError('targets %s (expected [N,C,r,r])' % (tuple(targets.shape),))
        N = targets.shape[0]
        if z0 is None:
            from .utils import device_latents
            z = device_latents(N, net.latent_size, seed=self.seed, device=targets.device)()
        else:
            z = engine._check_dev(z0, 'z0').clone()
        z, targets = self._check(net, z, targets)
        m, v = torch.zeros_like(z), torch.zeros_like(z)
        history = torch.empty((self.steps, N), device=z.device, dtype=torch.float32)
        b1, b2 = self.betas
        for t in range(self.steps):
            loss, dz = self.loss_and_grad(z, targets)
            history[t].copy_(loss)
            ops.adam(z.view(-1), dz.view(-1), m.view(-1), v.view(-1), self.learning_rate(t), b1, b2, self.eps,
                     1.0 - b1 ** (t + 1), math.sqrt(1.0 - b2 ** (t + 1)))
        images = engine.generator_forward(net, z)
        loss, _ = self._pyramid(images, targets, False)
        return Projection(z=z, images=images, loss=loss, history=history)
