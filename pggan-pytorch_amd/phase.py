"""Tensor-level wrappers of the magnitude + instantaneous-frequency kernels (include/pggan_hip_phase.h, csrc/phase.hip): the sound ends
that keep the phase (after Engel et al. 2019, GANSynth; DESIGN.md section 7 has the definitions).

  * ``analyse``     waveforms -> ``logmag = log1p(|STFT|)`` and ``ifreq``, the wrapped frame-to-frame difference of the phase in units
                    of pi, float64 ``[batch, bins, frames]``
  * ``magif_u8``    both planes -> the two-channel uint8 image ``[batch, 2, bins, frames]`` (256 levels on the IF circle, 128 = 0)
  * ``spectrum`` / ``pieces`` / ``synthesise``   a two-channel fp32 image -> complex spectrum (magnitude from channel 0, the running
                    sum of channel 1 as phase) -> windowed inverse transforms -> ``ops.overlap_add`` -> float64 waveforms

PyTorch is the allocator and the stream provider, as in ops.py: device tensors in and out, every launch on the current stream, no host
synchronisation, no CPU fallback (``sound.SoundSaver(mode='magif')`` is the numpy twin)."""
import math

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
