"""Differentiable augmentation of everything the discriminator sees (include/pggan_hip_augment.h has the definition).

``Augmenter`` is the policy and its state: the probability ``p`` (mutable: ``plugins.AugmentController`` steers it), the seed with one
draw counter per step kind, and the fp64 accumulator the controller reads.  ``gan_losses(..., augment=aug)`` puts it into the step's
``engine.Objective``: reals and fakes are augmented in the D step, fakes in the G step, and the G step's image gradient goes back through
the exact transpose (``adjoint``) into the generator -- DiffAugment (Zhao et al. 2020) with the adaptive probability of ADA (Karras et
al. 2020).  For sound: a shift in time (and, on request, in frequency), a cutout that is SpecAugment's time / frequency mask at ratio 1.0
on one axis, a gain on the log-magnitude channel, an x-flip.

A step's parameters are one int32 table [rows, 8], a row per image: ``(flags, dy, dx, y0, y1, x0, x1, gain_bits)``.  ``table`` makes the
next one from U[0,1) draws of the counter-based generator (``ops.uniform_``: element e of draw number d under ``seed``), so a table is a
pure function of (seed, counter, policy, p).  The D steps draw the even draw numbers and the G steps the odd ones: the two streams do not
depend on how the steps interleave.  Under data parallelism every rank passes ``seed=parallel.shard_seed(seed, rank)``.

``device='cpu'`` is the numpy twin of all of it, bit for bit (host mode: ``uniform_host``, ``table_host``, ``apply_host``,
``adjoint_host`` below; tensors in, CPU tensors out)."""
import numpy as np
import torch

COLS, FLIP, GAIN = 8, 1, 2          # the table's layout and flag bits (include/pggan_hip_augment.h; held against the header by the host tests)
MAX_SIZE = 4096


# ------------------------------------------------------------------------------------------ the numpy twin
def uniform_host(seed, draw, n):
    """Elements 0 .. n - 1 of draw number ``draw`` under ``seed`` as pg_uniform_f32 makes them: Philox4x32-10 on the counter
    (element // 4, draw) with the key ``seed``, 24 bits -> [0, 1) float32."""
    m = np.uint64(0xffffffff)
    i4 = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    c = [i4 & m, i4 >> np.uint64(32), np.full_like(i4, draw & 0xffffffff), np.full_like(i4, draw >> 32)]
    k = [seed & 0xffffffff, seed >> 32]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & m]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    bits = np.stack(c, axis=1).reshape(-1)[:int(n)]
    return (bits >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def table_host(U, H, W, ry, rx, ch, cw, gain, flip, p):
    """pg_augment_table in numpy float32, operation by operation (one rounding each, a floor behind every product): U [rows, 8] -> int32 [rows, 8]."""
    f32 = np.float32
    U = np.ascontiguousarray(U, dtype=np.float32).reshape(-1, COLS)
    u = [U[:, k] for k in range(COLS)]
    ry, rx, ch, cw, gain, p, fH, fW = f32(ry), f32(rx), f32(ch), f32(cw), f32(gain), f32(p), f32(H), f32(W)
    rows = U.shape[0]
    out = np.zeros((rows, COLS), dtype=np.int32)
    if flip:
        out[:, 0] |= np.where((u[0] < p) & (u[1] < f32(0.5)), FLIP, 0).astype(np.int32)
    shift = u[2] < p
    my, mx = int(np.floor(ry * fH)), int(np.floor(rx * fW))
    dy = np.minimum(np.floor(u[3] * f32(2 * my + 1)).astype(np.int32), 2 * my) - my
    dx = np.minimum(np.floor(u[4] * f32(2 * mx + 1)).astype(np.int32), 2 * mx) - mx
    out[:, 1], out[:, 2] = np.where(shift, dy, 0), np.where(shift, dx, 0)
    hc, wc = int(np.floor(ch * fH + f32(0.5))), int(np.floor(cw * fW + f32(0.5)))
    if hc > 0 and wc > 0:
        cut = u[5] < p
        t = u[6] * f32(4096.0)
        f = np.floor(t)
        cy = np.floor((f * f32(1.0 / 4096.0)) * fH).astype(np.int32)
        cx = np.floor((t - f) * fW).astype(np.int32)

        def axis(centre, n, size):
            if n >= size:
                return np.zeros(rows, np.int32), np.full(rows, size, np.int32)
            return np.maximum(centre - n // 2, 0), np.minimum(centre - n // 2 + n, size)
        (y0, y1), (x0, x1) = axis(cy, hc, int(H)), axis(cx, wc, int(W))
        for col, v in zip((3, 4, 5, 6), (y0, y1, x0, x1)):
            out[:, col] = np.where(cut, v, 0)
    if gain > 0:
        on = u[7] < p
        t = f32(2.0) * u[1]
        ug = t - np.floor(t)
        b = ((f32(2.0) * ug - f32(1.0)) * gain).astype(np.float32)
        out[:, 0] |= np.where(on, GAIN, 0).astype(np.int32)
        out[:, 7] = np.where(on, b.view(np.int32), 0)
    return out


def _grids(row, H, W, adjoint):
    """(source row index, source column index, live mask) [H, W] of one image under the table row ``row``."""
    flags, dy, dx, y0, y1, x0, x1 = (int(v) for v in row[:7])
    i, j = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing='ij')
    if not adjoint:                                  # output pixel (i, j) reads (i - dy, j' - dx)
        jp = W - 1 - j if flags & FLIP else j
        si, sj = i - dy, jp - dx
        inside = (si >= 0) & (si < H) & (sj >= 0) & (sj < W)
        ci, cj = i, j                                # the cutout lives in the augmented image: the output here ...
    else:                                            # input pixel (r, s) is the source of (r + dy, j) with j' = s + dx
        si, jp = i + dy, j + dx
        sj = W - 1 - jp if flags & FLIP else jp
        inside = (si >= 0) & (si < H) & (jp >= 0) & (jp < W)
        ci, cj = si, sj                              # ... and the pixel that is read in the transpose
    cut = (ci >= y0) & (ci < y1) & (cj >= x0) & (cj < x1)
    return np.clip(si, 0, H - 1), np.clip(sj, 0, W - 1), inside & ~cut


def _gather_host(x, table, adjoint, channel_mask):
    x = np.ascontiguousarray(x, dtype=np.float32)
    table = np.ascontiguousarray(table, dtype=np.int32)
    N, C, H, W = x.shape
    if table.shape != (N, COLS):
        raise ValueError('the table must be int32 [%d, %d], got %s' % (N, COLS, table.shape))
    bits = x.view(np.uint32)
    out = np.zeros_like(bits)
    for n in range(N):
        si, sj, live = _grids(table[n], H, W, adjoint)
        src = bits[n][:, si, sj]                                               # [C, H, W]
        out[n] = np.where(live[None], src, np.uint32(0))
        if not adjoint and int(table[n, 0]) & GAIN:
            b = table[n, 7:8].view(np.float32)[0]
            for c in range(C):
                if (channel_mask >> c) & 1:
                    out[n, c] = np.where(live, (src[c].view(np.float32) + b).astype(np.float32).view(np.uint32), np.uint32(0))
    return out.view(np.float32)


def apply_host(x, table, channel_mask=0):
    """pg_augment_apply in numpy: bit for bit (the values travel as uint32; the gain is one float32 add)."""
    return _gather_host(x, table, False, int(channel_mask))


def adjoint_host(g, table):
    """pg_augment_adjoint in numpy: the exact transpose of ``apply_host`` under the same table."""
    return _gather_host(g, table, True, 0)


# ------------------------------------------------------------------------------------------ the policy and its state
def _ratio(v, what):
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError('Augmenter: %s = %r outside [0, 1]' % (what, v))
    return v


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


class Augmenter(object):
    """``Augmenter(p=1.0, translate=(ry, rx), cutout=(ch, cw), gain=g, gain_channels=(0,), flip=False, seed=0, device='cuda')``.

    Every operation of an image is enabled with probability ``p``, independently: a shift by up to ``floor(ry H)`` rows and
    ``floor(rx W)`` columns with zero padding (the default shifts in time only: a shift in frequency is a pitch change), a cutout of
    ``round(ch H)`` x ``round(cw W)`` pixels centred uniformly over the image and clipped to it (ratio 1.0 on an axis masks the whole
    axis), a gain ``b`` uniform in [-g, g) added to the channels ``gain_channels``, an x-flip (with a further probability 1/2).
    ValueError for a ratio or ``p`` outside [0, 1] and for a negative gain.  Hashed by identity: it is part of the plans' keys."""

    def __init__(self, p=1.0, translate=(0.0, 0.125), cutout=(0.0, 0.0), gain=0.0, gain_channels=(0,), flip=False, seed=0, device='cuda'):
        self.p = _ratio(p, 'p')
        self.translate = (_ratio(translate[0], 'translate[0]'), _ratio(translate[1], 'translate[1]'))
        self.cutout = (_ratio(cutout[0], 'cutout[0]'), _ratio(cutout[1], 'cutout[1]'))
        self.gain = float(gain)
        if not self.gain >= 0.0 or self.gain == float('inf'):
            raise ValueError('Augmenter: gain = %r must be a finite number >= 0' % (gain,))
        self.gain_channels = tuple(int(c) for c in gain_channels)
        if any(not 0 <= c < 32 for c in self.gain_channels):
            raise ValueError('Augmenter: gain_channels %r outside 0 .. 31' % (gain_channels,))
        self.channel_mask = sum(1 << c for c in set(self.gain_channels))
        self.flip = bool(flip)
        self.seed = int(seed)
        self.draws = {'d': 0, 'g': 0}                 # tables drawn so far for D steps / for G steps
        self.device = torch.device(device)
        self.host = self.device.type == 'cpu'
        self.acc = torch.zeros(2, dtype=torch.float64, device=self.device)      # (sum of sign(real scores), real scores seen): pg_score_signs
        self.controller = None                        # plugins.AugmentController attaches itself: the D steps then count signs into ``acc``
        self.kind = None                              # the kind of the objective ``gan_losses(..., augment=self)`` built (None: not handed to one yet)
        self._injected = {'d': None, 'g': None}

    # ---- tables
    def _check_p(self):
        p = float(self.p)
        if not 0.0 <= p <= 1.0:
            raise ValueError('Augmenter: p = %r outside [0, 1]' % (self.p,))
        return p

    def table(self, rows, H, W, which):
        """The next table [rows, 8] for images H x W of the ``which`` ('d' | 'g') stream: draw number ``2 k`` ('d') or ``2 k + 1`` ('g') for
        the k-th table of that stream, at the current ``p``.  Two launches on the current stream (the uniforms, the table); no host sync."""
        if which not in self.draws:
            raise ValueError("Augmenter.table: which = %r ('d' or 'g')" % (which,))
        rows, H, W, p = int(rows), int(H), int(W), self._check_p()
        if rows < 1 or min(H, W) < 4 or max(H, W) > MAX_SIZE or H & (H - 1) or W & (W - 1):
            raise ValueError('Augmenter.table: %d rows for images %d x %d (powers of two in 4 .. %d)' % (rows, H, W, MAX_SIZE))
        draw = 2 * self.draws[which] + (which == 'g')
        self.draws[which] += 1
        (ry, rx), (ch, cw) = self.translate, self.cutout
        if self.host:
            U = uniform_host(self.seed, draw, rows * COLS).reshape(rows, COLS)
            return torch.from_numpy(table_host(U, H, W, ry, rx, ch, cw, self.gain, self.flip, p))
        from . import ops
        U = ops.uniform_(torch.empty((rows, COLS), device=self.device, dtype=torch.float32), self.seed, draw)
        return ops.augment_table(U, H, W, ry, rx, ch, cw, self.gain, self.flip, p)

    def inject(self, d_table=None, g_table=None):
        """Hand the NEXT D loss (``d_table`` [2N, 8]: reals, then fakes) or G loss (``g_table`` [N, 8]) this table instead of a draw; it is
        consumed by that loss and draws nothing (parity tests, as ``wgan_gp_loss.set_mixing_factors`` for the mixing factors)."""
        if d_table is not None:
            self._injected['d'] = d_table
        if g_table is not None:
            self._injected['g'] = g_table

    def next_table(self, which, rows, H, W):
        """What a loss call takes: the injected table of its stream, consumed, or else ``table(...)``."""
        t, self._injected[which] = self._injected[which], None
        if t is None:
            return self.table(rows, H, W, which)
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32))
        t = t.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(t.shape) != (rows, COLS):
            raise ValueError('Augmenter: the injected table is %s, the step needs [%d, %d]' % (tuple(t.shape), rows, COLS))
        return t

    # ---- the gather and its transpose
    def apply(self, x, table, out=None):
        """``x`` [N,C,H,W] as D sees it under ``table`` [N, 8]."""
        if self.host:
            y = torch.from_numpy(apply_host(_np(x), _np(table), self.channel_mask))
            return y if out is None else out.copy_(y)
        from . import ops
        return ops.augment_apply(x, table, self.channel_mask, out=out)

    def adjoint(self, g, table, out=None):
        """The transpose of ``apply`` under the same table: the gradient with respect to ``x`` from the one with respect to ``apply(x)``."""
        if self.host:
            y = torch.from_numpy(adjoint_host(_np(g), _np(table)))
            return y if out is None else out.copy_(y)
        from . import ops
        return ops.augment_adjoint(g, table, out=out)

    # ---- the overfitting signal
    def read(self):
        """(sum of the signs of the real scores, real scores counted) so far, as Python floats: the one host synchronisation of the feature."""
        a = self.acc.cpu()
        return float(a[0]), float(a[1])
