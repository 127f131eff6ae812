"""Tensor-level wrappers of the magnitude + instantaneous-frequency kernels (include/pggan_hip_phase.h, csrc/phase.hip): the sound ends
that keep the phase (after Engel et al. 2019, GANSynth; DESIGN.md section 7 has the definitions).

  * ``analyse``     waveforms -> ``logmag = log1p(|STFT|)`` and ``ifreq``, the wrapped frame-to-frame difference of the phase in units
                    of pi, float64 ``[batch, bins, frames]``
  * ``magif_u8``    both planes -> the two-channel uint8 image ``[batch, 2, bins, frames]`` (256 levels on the IF circle, 128 = 0)
  * ``spectrum`` / ``pieces`` / ``synthesise``   a two-channel fp32 image -> complex spectrum (magnitude from channel 0, the running
                    sum of channel 1 as phase) -> windowed inverse transforms -> ``ops.overlap_add`` -> float64 waveforms
  * ``MelTable`` / ``mel_table``, ``mel_analyse`` / ``mel_spectrum`` / ``mel_synthesise``   the same on M mel-spaced rows made from
                    the n_fft/2 >= M bins of a longer transform ('melif'; include/pggan_hip_mel.h, csrc/mel.hip)

PyTorch is the allocator and the stream provider, as in ops.py: device tensors in and out, every launch on the current stream, no host
synchronisation, no CPU fallback (``sound.SoundSaver(mode='magif')`` is the numpy twin)."""
import functools
import math

import numpy as np
import torch

from . import _lib, ops
from .ops import _stream, require_gpu, _f32_dev, _f64_dev

_C = _lib.PHASE_CONSTANTS          # every #define PG_* that include/pggan_hip_phase.h carries

MIN_N, MAX_N = _C['PG_PHASE_MIN_N'], _C['PG_PHASE_MAX_N']       # n_fft = 2 H: a power of two in this range (image heights 4 .. 1024)
IF_LEVELS, IF_ZERO = _C['PG_PHASE_IF_LEVELS'], _C['PG_PHASE_IF_ZERO']


def default_mag_range(n_fft):
    """(0, log1p(n_fft/2)): never clipped for |y| <= 1, because |S| <= sum(window) = n_fft/2.  Fixed, not a per-file min/max, so that
    the image can be inverted."""
    return (0.0, math.log1p(n_fft // 2))


def check_mag_range(mag_range, n_fft, what):
    if mag_range is None:
        return default_mag_range(n_fft)
    try:
        lo, hi = (float(v) for v in mag_range)
    except (TypeError, ValueError):
        raise ValueError('%s: mag_range must be None or (lo, hi), got %r' % (what, mag_range))
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError('%s: mag_range must be finite with hi > lo, got %r' % (what, mag_range))
    return (lo, hi)


def _n_fft(n_fft, what):
    if isinstance(n_fft, bool) or int(n_fft) != n_fft or n_fft < MIN_N or n_fft > MAX_N or int(n_fft) & (int(n_fft) - 1):
        raise ValueError('%s: n_fft must be a power of two in %d .. %d, got %r' % (what, MIN_N, MAX_N, n_fft))
    return int(n_fft)


def _range(range_in, range_out):
    """(lo_in, scale, lo_out) of adjust_dynamic_range (utils.py:24-30), which leaves equal ranges untouched."""
    if tuple(range_in) == tuple(range_out):
        return 0.0, 1.0, 0.0
    return float(range_in[0]), (range_out[1] - range_out[0]) / (range_in[1] - range_in[0]), float(range_out[0])


def analyse(signals, n_fft, hop_length, bins=None, frames=None):
    """fp32 device waveforms ``[batch, nsamp]`` (or ``[nsamp]``) -> ``(logmag, ifreq)`` float64 ``[batch, bins, frames]``
    (pg_phase_analyse_f64, one launch).  ``bins`` <= n_fft/2 + 1 (default: all) and ``frames`` <= 1 + nsamp // hop_length (default: all):
    only what is asked for is computed.  nsamp > n_fft/2."""
    _f32_dev(signals, 'analyse signals')
    if signals.dim() == 1:
        signals = signals[None]
    if signals.dim() != 2 or signals.shape[0] < 1:
        raise ValueError('analyse signals: expected [batch, nsamp] or [nsamp], got shape %s' % (tuple(signals.shape),))
    n_fft, hop = _n_fft(n_fft, 'analyse'), int(hop_length)
    batch, nsamp = signals.shape
    if hop < 1 or batch > 65535:
        raise ValueError('analyse: hop_length must be >= 1 and the batch at most 65535')
    if nsamp <= n_fft // 2:
        raise ValueError('analyse: %d samples, reflect padding by n_fft/2 = %d needs more' % (nsamp, n_fft // 2))
    bins = n_fft // 2 + 1 if bins is None else int(bins)
    frames = 1 + nsamp // hop if frames is None else int(frames)
    if not 1 <= bins <= n_fft // 2 + 1 or not 1 <= frames <= 1 + nsamp // hop:
        raise ValueError('analyse: bins %d of %d, frames %d of %d' % (bins, n_fft // 2 + 1, frames, 1 + nsamp // hop))
    require_gpu()
    logmag = torch.empty((batch, bins, frames), device=signals.device, dtype=torch.float64)
    ifreq = torch.empty((batch, bins, frames), device=signals.device, dtype=torch.float64)
    _lib.call('pg_phase_analyse_f64', signals.data_ptr(), nsamp, batch, logmag.data_ptr(), ifreq.data_ptr(), n_fft, hop, bins, frames,
              _stream())
    return logmag, ifreq


def magif_u8(logmag, ifreq, mag_range):
    """float64 device planes ``[batch, bins, frames]`` of ``analyse`` -> uint8 ``[batch, 2, bins, frames]`` (pg_phase_quantise_u8, one
    launch): channel 0 = clip(rint((logmag - lo) / (hi - lo) * 255), 0, 255), channel 1 = rint((ifreq + 1) * 128) mod 256."""
    _f64_dev(logmag, 'magif_u8 logmag', 3)
    _f64_dev(ifreq, 'magif_u8 ifreq', 3)
    if logmag.shape != ifreq.shape or logmag.device != ifreq.device or logmag.numel() < 1:
        raise ValueError('magif_u8: logmag %s and ifreq %s must be non-empty, of one shape and on one device'
                         % (tuple(logmag.shape), tuple(ifreq.shape)))
    if mag_range is None:
        raise ValueError('magif_u8: mag_range must be (lo, hi), e.g. default_mag_range(n_fft)')
    lo, hi = check_mag_range(mag_range, None, 'magif_u8')
    batch, bins, frames = logmag.shape
    out = torch.empty((batch, 2, bins, frames), device=logmag.device, dtype=torch.uint8)
    _lib.call('pg_phase_quantise_u8', logmag.data_ptr(), ifreq.data_ptr(), out.data_ptr(), batch, bins * frames, lo, hi, _stream())
    return out


def _images(images, what):
    _f32_dev(images, what + ' images', 4)
    n, C, H, W = images.shape
    if n < 1 or n > 65535 or C != 2:
        raise ValueError('%s images: expected [n,2,H,W] with 1 <= n <= 65535, got shape %s' % (what, tuple(images.shape)))
    if H != W or H & (H - 1) or not MIN_N <= 2 * H <= MAX_N:
        raise ValueError('%s images: must be square with a power-of-two side in %d .. %d, got %dx%d' % (what, MIN_N // 2, MAX_N // 2, H, W))
    return n, H, W


def spectrum(images, drange=(-1, 1), mag_range=None, return_phase=False):
    """fp32 device images ``[n, 2, H, W]`` -> the complex128 spectrum ``[n, W frames, H + 1 bins]`` (pg_phase_spectrum_f64, one launch):
    ``mag = expm1(max(adjust_dynamic_range(img[0], drange, mag_range), 0))``, ``ifreq = adjust_dynamic_range(img[1], drange, (0, 255))
    / 128 - 1`` (not clamped), ``c`` = its running sum along W, ``spec = mag * (cospi(c), sinpi(c))``; the bin H (Nyquist) is 0.
    ``return_phase``: also ``c`` itself, float64 ``[n, H, W]``."""
    n, H, W = _images(images, 'spectrum')
    mag_range = check_mag_range(mag_range, 2 * H, 'spectrum')
    rm, rf = _range(drange, mag_range), _range(drange, (0, 255))
    spec = torch.empty((n, W, H + 1, 2), device=images.device, dtype=torch.float64)
    csum = torch.empty((n, H, W), device=images.device, dtype=torch.float64) if return_phase else None
    _lib.call('pg_phase_spectrum_f64', images.data_ptr(), spec.data_ptr(), None if csum is None else csum.data_ptr(), n, H, W,
              rm[0], rm[1], rm[2], rf[0], rf[1], rf[2], _stream())
    spec = torch.view_as_complex(spec)
    return (spec, csum) if return_phase else spec


def pieces(spec):
    """complex128 device spectrum ``[batch, frames, n_fft/2 + 1]`` -> float64 ``[batch, frames, n_fft]`` (pg_phase_pieces_f64, one launch):
    irfft of every frame (the imaginary parts of DC and Nyquist are ignored) x window x 2/3, the summands of ``ops.overlap_add``."""
    if not torch.is_tensor(spec) or not spec.is_cuda or spec.dtype != torch.complex128 or not spec.is_contiguous() or spec.dim() != 3:
        raise ValueError('pieces spec: expected a contiguous complex128 device tensor [batch, frames, n_fft/2 + 1]')
    batch, frames, bins = spec.shape
    n_fft = _n_fft(2 * (bins - 1), 'pieces')
    if batch < 1 or batch > 65535 or frames < 1 or frames * batch > 1 << 22:
        raise ValueError('pieces spec: batch %d (1 .. 65535), frames %d (frames x batch <= 2^22)' % (batch, frames))
    out = torch.empty((batch, frames, n_fft), device=spec.device, dtype=torch.float64)
    _lib.call('pg_phase_pieces_f64', torch.view_as_real(spec).data_ptr(), out.data_ptr(), n_fft, frames, batch, _stream())
    return out


def synthesise(images, hop_length, drange=(-1, 1), mag_range=None):
    """fp32 device images ``[n, 2, H, W]`` -> float64 device waveforms ``[n, hop_length (W - 1)]``: ``spectrum``, ``pieces`` and
    ``ops.overlap_add``, three launches and one inverse STFT where 'abslog' needs Griffin-Lim's rounds.  Peak normalisation and repeat
    are ``ops.wave_normalize``."""
    n, H, W = _images(images, 'synthesise')
    hop = int(hop_length)
    if hop < 1:
        raise ValueError('synthesise: hop_length must be >= 1')
    return ops.overlap_add(pieces(spectrum(images, drange, mag_range)), hop)


def spectrogram_stack_u8(signals, n_fft, hop_length, mag_range=None):
    """fp32 device waveforms ``[batch, nsamp]`` -> uint8 ``[batch, 2, n_fft/2, n_fft/2]`` 'magif' images, the first n_fft/2 bins and
    frames: ``analyse`` and ``magif_u8``, for filling a ``DeviceImageDataset`` stack."""
    n_fft = _n_fft(n_fft, 'spectrogram_stack_u8')
    mag_range = check_mag_range(mag_range, n_fft, 'spectrogram_stack_u8')
    _f32_dev(signals, 'spectrogram_stack_u8 signals', 2)
    side, nsamp = n_fft // 2, signals.shape[1]
    if int(hop_length) < 1 or 1 + nsamp // int(hop_length) < side:
        raise ValueError('spectrogram_stack_u8: %d samples every %r give too few frames, the %dx%d image needs %d'
                         % (nsamp, hop_length, side, side, side))
    logmag, ifreq = analyse(signals, n_fft, hop_length, side, side)
    return magif_u8(logmag, ifreq, mag_range)


def real_batch_2ch_u8(stack_u8, idx, flip, depthdiff, alpha, range_in, range_out):
    """``ops.real_batch_u8`` for a checked two-channel stack (pg_real_batch_2ch_u8: the same kernels with C = 2)."""
    M, C, S, _ = stack_u8.shape
    r = S >> depthdiff if 0 <= depthdiff < 31 else 0
    out = torch.empty((idx.numel(), C, r, r), device=stack_u8.device, dtype=torch.float32)
    _lib.call('pg_real_batch_2ch_u8', stack_u8.data_ptr(), M, S, depthdiff, idx.data_ptr(), None if flip is None else flip.data_ptr(),
              idx.numel(), out.data_ptr(), float(alpha), float(range_in[0]), float(range_in[1]), float(range_out[0]), float(range_out[1]),
              _stream())
    return out


# ------------------------------------------------------------------ 'melif': the same two planes on warped (mel) rows (csrc/mel.hip)
def _mel(f):
    return 1127.0 * np.log1p(np.asarray(f, dtype=np.float64) / 700.0)


def _mel_inverse(m):
    return 700.0 * np.expm1(np.asarray(m, dtype=np.float64) / 1127.0)


def mel_positions(n_fft, rows, sample_rate):
    """``(p, q)`` of DESIGN.md section 7: the centres ``p[m]`` of the ``rows`` image rows in units of bins, equally spaced in
    mel(f) = 1127 log1p(f / 700) from bin 0 to bin H - 1 = n_fft/2 - 1, and the position ``q[k]`` of every bin in units of rows.  The
    end points are exact.  numpy fp64."""
    H, M, sr = n_fft // 2, int(rows), float(sample_rate)
    top = _mel((H - 1) * sr / n_fft)
    p = _mel_inverse(np.arange(M) * top / (M - 1)) * n_fft / sr
    p[0], p[-1] = 0.0, float(H - 1)
    q = _mel(np.arange(H) * sr / n_fft) / top * (M - 1)
    q[0], q[-1] = 0.0, float(M - 1)
    return p, q


def _mel_arrays(n_fft, rows, sample_rate):
    """The arrays of ``mel_table``: triangles around ``p[m]`` that reach to the neighbouring centres but never less than ONE bin to
    either side, normalised to sum 1 -- where the rows are closer than the bins a row is the linear interpolation of its two
    neighbouring bins and never empty, where they are wider it is a triangle over its band; and ``(floor(q), q - floor(q))``."""
    H, M = n_fft // 2, int(rows)
    p, q = mel_positions(n_fft, rows, sample_rate)
    gap = np.diff(p)
    left = np.maximum(np.concatenate([gap[:1], gap]), 1.0)
    right = np.maximum(np.concatenate([gap, gap[-1:]]), 1.0)
    k = np.arange(H, dtype=np.float64)
    start, count, weights = [], [], []
    for m in range(M):
        d = k - p[m]
        w = np.maximum(0.0, np.where(d <= 0, 1.0 + d / left[m], 1.0 - d / right[m]))
        nz = np.flatnonzero(w)
        w = w[nz[0]:nz[-1] + 1]
        start.append(nz[0])
        count.append(len(w))
        weights.append(w / w.sum())
    lower = np.minimum(np.floor(q), M - 2)
    return start, count, np.concatenate(weights), lower.astype(np.int64), q - lower


class MelTable(object):
    """The warp between the H = n_fft/2 linear bins of a transform and the ``rows`` <= H rows of a 'melif' image, as plain arrays
    (include/pggan_hip_mel.h): the kernels take ANY table of this shape.

      start, count  int [rows]: row m weighs the bins start[m] .. start[m] + count[m] - 1, inside [0, H), count >= 1
      weights       float64 [sum(count)], row after row, finite (``mel_table`` makes every row sum to 1)
      lower, frac   int [H] in [0, rows - 2] and float64 [H] in [0, 1]: bin k lies between rows lower[k] and lower[k] + 1

    A malformed array is a ValueError here, once: the kernels do not check.  The arrays live on the host (read-only numpy) and are
    uploaded to a device at first use there (``on``)."""

    def __init__(self, n_fft, start, count, weights, lower, frac):
        self.n_fft = _n_fft(n_fft, 'MelTable')
        H = self.bins = self.n_fft // 2
        try:
            start, count, lower = (np.array(a) for a in (start, count, lower))
            weights, frac = np.array(weights, dtype=np.float64), np.array(frac, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('MelTable: start, count, weights, lower and frac must be arrays of numbers')
        for name, a in (('start', start), ('count', count), ('lower', lower)):
            if a.ndim != 1 or a.dtype.kind not in 'iu':
                raise ValueError('MelTable: %s must be a one-dimensional integer array' % name)
        M = self.rows = int(start.shape[0])
        if not 2 <= M <= H or count.shape != (M,):
            raise ValueError('MelTable: start and count must have one length in 2 .. n_fft/2 = %d, got %d and %d' % (H, M, count.shape[0]))
        if (count < 1).any() or (start < 0).any() or (start.astype(np.int64) + count > H).any():
            raise ValueError('MelTable: every band must have count >= 1 and lie inside [0, %d)' % H)
        if weights.ndim != 1 or weights.shape[0] != int(count.sum()) or not np.isfinite(weights).all():
            raise ValueError('MelTable: weights must be sum(count) = %d finite numbers' % int(count.sum()))
        if lower.shape != (H,) or frac.shape != (H,):
            raise ValueError('MelTable: lower and frac must have n_fft/2 = %d entries' % H)
        if (lower < 0).any() or (lower > M - 2).any():
            raise ValueError('MelTable: lower must lie in [0, rows - 2] = [0, %d]' % (M - 2))
        if not ((frac >= 0) & (frac <= 1)).all():                            # (refuses NaN too)
            raise ValueError('MelTable: frac must lie in [0, 1]')
        self.start, self.count, self.lower = (a.astype(np.int32) for a in (start, count, lower))
        self.offset = (np.cumsum(self.count, dtype=np.int64) - self.count).astype(np.int32)
        self.weights, self.frac = weights, frac
        for a in (self.start, self.count, self.offset, self.lower, self.weights, self.frac):
            a.setflags(write=False)
        self._on = {}

    @classmethod
    def identity(cls, n_fft):
        """rows = n_fft/2, row m is bin m: ``mel_analyse`` / ``mel_spectrum`` then give the bits of ``analyse(bins=n_fft/2)`` /
        ``spectrum``.  (The last bin sits on the last row as frac 1 above row rows - 2: lower stays inside [0, rows - 2].)"""
        H = _n_fft(n_fft, 'MelTable.identity') // 2
        frac = np.zeros(H)
        frac[-1] = 1.0
        return cls(n_fft, np.arange(H), np.ones(H, dtype=np.int64), np.ones(H), np.minimum(np.arange(H), H - 2), frac)

    def row_weights(self, m):
        return self.weights[self.offset[m]:self.offset[m] + self.count[m]]

    def on(self, device):
        """The six arrays on ``device`` (uploaded once per device): start, count, offset, weights, lower, frac.  The first use on a
        device is a host-to-device copy from pageable memory: before capturing a graph (``torch.cuda.graph``) that contains
        ``mel_analyse`` / ``mel_spectrum``, call ``table.on(device)`` once outside the capture."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = tuple(torch.from_numpy(np.array(a)).to(device)
                                     for a in (self.start, self.count, self.offset, self.weights, self.lower, self.frac))
        return self._on[device]


@functools.lru_cache(maxsize=None)
def _mel_table(n_fft, rows, sample_rate):
    return MelTable(n_fft, *_mel_arrays(n_fft, rows, sample_rate))


def mel_table(n_fft, rows, sample_rate=16000):
    """The mel ``MelTable`` of ``rows`` image rows (a power of two, 4 <= rows <= n_fft/2) over the n_fft/2 bins of an ``n_fft``-point
    transform at ``sample_rate`` Hz (``_mel_arrays``).  Built once per (n_fft, rows, sample_rate) and kept."""
    n_fft = _n_fft(n_fft, 'mel_table')
    if isinstance(rows, bool) or int(rows) != rows or rows < 4 or rows > n_fft // 2 or int(rows) & (int(rows) - 1):
        raise ValueError('mel_table: rows must be a power of two in 4 .. n_fft/2 = %d, got %r' % (n_fft // 2, rows))
    try:
        sr = float(sample_rate)
    except (TypeError, ValueError):
        sr = float('nan')
    if isinstance(sample_rate, bool) or not (math.isfinite(sr) and sr > 0):
        raise ValueError('mel_table: sample_rate must be a positive number, got %r' % (sample_rate,))
    return _mel_table(n_fft, int(rows), sr)


def _table(table, what):
    if not isinstance(table, MelTable):
        raise ValueError('%s: table must be a MelTable (mel_table(n_fft, rows, sample_rate)), got %r' % (what, type(table).__name__))
    return table


def mel_analyse(signals, n_fft, hop_length, table, frames=None):
    """fp32 device waveforms ``[batch, nsamp]`` (or ``[nsamp]``) -> ``(logmag, ifreq)`` float64 ``[batch, table.rows, frames]``
    (pg_mel_analyse_f64, one launch): ``analyse`` with every row the weighted mean magnitude (then log1p) and the magnitude-weighted
    circular mean of the IF over its band of bins; a one-bin row is that bin.  ``frames`` <= 1 + nsamp // hop_length (default: all)."""
    _f32_dev(signals, 'mel_analyse signals')
    if signals.dim() == 1:
        signals = signals[None]
    if signals.dim() != 2 or signals.shape[0] < 1:
        raise ValueError('mel_analyse signals: expected [batch, nsamp] or [nsamp], got shape %s' % (tuple(signals.shape),))
    n_fft, hop = _n_fft(n_fft, 'mel_analyse'), int(hop_length)
    if _table(table, 'mel_analyse').n_fft != n_fft:
        raise ValueError('mel_analyse: the table is for n_fft %d, not %d' % (table.n_fft, n_fft))
    batch, nsamp = signals.shape
    if hop < 1 or batch > 65535:
        raise ValueError('mel_analyse: hop_length must be >= 1 and the batch at most 65535')
    if nsamp <= n_fft // 2:
        raise ValueError('mel_analyse: %d samples, reflect padding by n_fft/2 = %d needs more' % (nsamp, n_fft // 2))
    frames = 1 + nsamp // hop if frames is None else int(frames)
    if not 1 <= frames <= 1 + nsamp // hop:
        raise ValueError('mel_analyse: frames %d of %d' % (frames, 1 + nsamp // hop))
    require_gpu()
    start, count, offset, weights, _, _ = table.on(signals.device)
    logmag = torch.empty((batch, table.rows, frames), device=signals.device, dtype=torch.float64)
    ifreq = torch.empty((batch, table.rows, frames), device=signals.device, dtype=torch.float64)
    _lib.call('pg_mel_analyse_f64', signals.data_ptr(), nsamp, batch, logmag.data_ptr(), ifreq.data_ptr(), n_fft, hop, table.rows, frames,
              start.data_ptr(), count.data_ptr(), offset.data_ptr(), weights.data_ptr(), _stream())
    return logmag, ifreq


def _mel_images(images, table, what):
    _f32_dev(images, what + ' images', 4)
    n, C, M, W = images.shape
    if n < 1 or n > 65535 or C != 2:
        raise ValueError('%s images: expected [n,2,M,W] with 1 <= n <= 65535, got shape %s' % (what, tuple(images.shape)))
    if M != W or M & (M - 1) or M < MIN_N // 2:
        raise ValueError('%s images: must be square with a power-of-two side >= %d, got %dx%d' % (what, MIN_N // 2, M, W))
    if _table(table, what).rows != M:
        raise ValueError('%s images: %d rows, the table has %d' % (what, M, table.rows))
    return n, M, W


def mel_spectrum(images, table, drange=(-1, 1), mag_range=None, return_phase=False):
    """fp32 device images ``[n, 2, M, W]`` -> the complex128 spectrum ``[n, W frames, H + 1 bins]`` of the H = table.bins linear bins
    (pg_mel_spectrum_f64, one launch): ``spectrum`` with the magnitude of bin k interpolated between rows ``lower[k]`` and
    ``lower[k] + 1`` and its IF along the shorter arc between theirs (frac 0 / 1: the one row alone).  ``mag_range`` defaults to
    ``default_mag_range(table.n_fft)``.  ``return_phase``: also the running sum ``c``, float64 ``[n, H, W]``."""
    n, M, W = _mel_images(images, table, 'mel_spectrum')
    H = table.bins
    mag_range = check_mag_range(mag_range, table.n_fft, 'mel_spectrum')
    rm, rf = _range(drange, mag_range), _range(drange, (0, 255))
    _, _, _, _, lower, frac = table.on(images.device)
    spec = torch.empty((n, W, H + 1, 2), device=images.device, dtype=torch.float64)
    csum = torch.empty((n, H, W), device=images.device, dtype=torch.float64) if return_phase else None
    _lib.call('pg_mel_spectrum_f64', images.data_ptr(), spec.data_ptr(), None if csum is None else csum.data_ptr(), n, M, H, W,
              lower.data_ptr(), frac.data_ptr(), rm[0], rm[1], rm[2], rf[0], rf[1], rf[2], _stream())
    spec = torch.view_as_complex(spec)
    return (spec, csum) if return_phase else spec


def mel_synthesise(images, hop_length, table, drange=(-1, 1), mag_range=None):
    """fp32 device images ``[n, 2, M, W]`` -> float64 device waveforms ``[n, hop_length (W - 1)]``: ``mel_spectrum``, ``pieces`` and
    ``ops.overlap_add`` with n_fft = table.n_fft, three launches as ``synthesise``."""
    _mel_images(images, table, 'mel_synthesise')
    hop = int(hop_length)
    if hop < 1:
        raise ValueError('mel_synthesise: hop_length must be >= 1')
    return ops.overlap_add(pieces(mel_spectrum(images, table, drange, mag_range)), hop)


def mel_spectrogram_stack_u8(signals, n_fft, hop_length, table, mag_range=None, frames=None):
    """fp32 device waveforms ``[batch, nsamp]`` -> uint8 ``[batch, 2, table.rows, frames]`` 'melif' images (``frames`` defaults to
    table.rows: square): ``mel_analyse`` and ``magif_u8``, two launches."""
    n_fft = _n_fft(n_fft, 'mel_spectrogram_stack_u8')
    mag_range = check_mag_range(mag_range, n_fft, 'mel_spectrogram_stack_u8')
    _f32_dev(signals, 'mel_spectrogram_stack_u8 signals', 2)
    frames, nsamp = _table(table, 'mel_spectrogram_stack_u8').rows if frames is None else int(frames), signals.shape[1]
    if int(hop_length) < 1 or 1 + nsamp // int(hop_length) < frames:
        raise ValueError('mel_spectrogram_stack_u8: %d samples every %r give too few frames, the image needs %d' % (nsamp, hop_length, frames))
    logmag, ifreq = mel_analyse(signals, n_fft, hop_length, table, frames)
    return magif_u8(logmag, ifreq, mag_range)
