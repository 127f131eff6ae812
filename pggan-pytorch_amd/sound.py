"""Sound ends of the path: the spectrogram input step on the device and the ``SoundSaver``
post-processor with the reference's hook signature.

  * ``spectrogram_u8`` — SoundImageDataset.load_file (/root/reference/dataset.py:285-300) for a waveform that is already in
    HBM: mono mix-down, STFT, crop, log(1 + |s|), stretch to uint8, by the HIP kernels of csrc/sound.hip.
  * ``SoundSaver`` — /root/reference/output_postprocess.py:75-153: ``proc(out, description)`` with ``out`` the fp32
    ``[n, 1, H, W]`` samples of G; 'abslog' images go through Griffin-Lim (``griffin_lim_iter`` rounds of STFT / inverse
    STFT), 'raw' images are the waveform itself; one 32-bit float WAV per sample, names as in the reference.  It runs on the
    host with numpy, as the reference does and as SURVEY.md §8f allows (6 samples every 3 ticks).
  * ``img_mode='magif'`` / ``mode='magif'`` — log-magnitude plus instantaneous frequency as a two-channel image (after Engel et al.
    2019, GANSynth): ``spectrogram_u8`` / ``spectrogram_stack_u8`` make the images (csrc/phase.hip), both savers
    turn them back into a waveform with one inverse STFT; the ``magif_*`` functions below are the definitions in numpy fp64.
  * ``img_mode='melif'`` / ``mode='melif'`` — the same two channels on M mel-spaced rows made from the n_fft/2 >= M bins of a longer
    transform (GANSynth's "IF-Mel + H"; DESIGN.md section 7, csrc/mel.hip): a 256^2 network can be fed from 1024 bins.  The warp is a
    table of plain arrays (``phase.mel_table``); the ``melif_*`` functions below are the definitions in numpy fp64.
  * ``DeviceSoundSaver`` — the same files from the device: the spectrum, every Griffin-Lim round and the normalisation are the fp64
    HIP kernels of csrc/griffinlim.hip; only the float32 waveforms are copied back.  Opt-in: ``SoundSaver`` stays the default.

The reference delegates the transforms to librosa 0.4.3 (requirements.txt:1), which is not in this image; both ends follow
its published definitions (periodic Hann window, center=True with reflect padding, hop_length; inverse: windowed
overlap-add with the 2/3 gain that makes hop = n_fft/4 an exact inverse).  Parity is therefore UNPINNED for these two
steps (no librosa, no reference vectors); ``oracle/sound_steps.py`` restates the same definitions independently and the
tests hold the two against each other plus the algebraic properties (inverse round trip, Griffin-Lim consistency)."""
import functools
import math
import os

import numpy as np

from . import _lib
from .utils import adjust_dynamic_range


MEL_SAMPLE_RATE = 16000               # the default ``sample_rate`` of img_mode='melif' (SoundSaver's default too)

# ------------------------------------------------------------------ rate conversion (include/pggan_hip_resample.h, csrc/resample.hip)
_RC = _lib.RESAMPLE_CONSTANTS
RESAMPLE_MAX_PHASES, RESAMPLE_MAX_TAPS = _RC['PG_RESAMPLE_MAX_PHASES'], _RC['PG_RESAMPLE_MAX_TAPS']
RESAMPLE_ZEROS, RESAMPLE_ROLLOFF, RESAMPLE_BETA = 64, 0.9475937167399596, 14.769656459379492     # resampy's published 'kaiser_best'


def _ratio(rate_in, rate_out):
    """(L, M) = (rate_out, rate_in) / gcd; the rates are positive integers (ValueError otherwise)."""
    for name, v in (('rate_in', rate_in), ('rate_out', rate_out)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('%s must be a positive integer (Hz), got %r' % (name, v))
    g = math.gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g


class ResampleTable(object):
    """The polyphase filter of ``resample`` as plain data (include/pggan_hip_resample.h): ``taps`` float64 ``[L, T]``, row r the T
    taps of phase r, T even; output n = (q L + r) / M weighs the samples q - T/2 + 1 .. q + T/2 with them.  The kernel and the numpy
    twin take ANY finite table of this shape (``resample_table`` builds the windowed sinc).  A malformed table is a ValueError here,
    once.  The array lives on the host (read-only numpy) and is uploaded to a device at first use there (``on``)."""

    def __init__(self, L, M, taps):
        for name, v in (('L', L), ('M', M)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError('ResampleTable: %s must be a positive integer, got %r' % (name, v))
        try:
            taps = np.array(taps, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('ResampleTable: taps must be an array of numbers [L, T]')
        if taps.ndim != 2 or taps.shape[0] != L or taps.shape[1] < 2 or taps.shape[1] % 2:
            raise ValueError('ResampleTable: taps must be [L = %d, T] with T even and >= 2, got shape %s' % (L, tuple(taps.shape)))
        if L > RESAMPLE_MAX_PHASES or taps.shape[1] > RESAMPLE_MAX_TAPS:
            raise ValueError('ResampleTable: %d phases of %d taps, at most %d and %d are supported (rates with a larger common divisor '
                             'give fewer phases)' % (L, taps.shape[1], RESAMPLE_MAX_PHASES, RESAMPLE_MAX_TAPS))
        if not np.isfinite(taps).all():
            raise ValueError('ResampleTable: taps must be finite')
        self.L, self.M, self.T = int(L), int(M), int(taps.shape[1])
        self.taps = np.ascontiguousarray(taps)
        self.taps.setflags(write=False)
        self._on = {}

    def on(self, device):
        """``taps`` on ``device`` (uploaded once per device; a host-to-device copy from pageable memory, so call it once outside a
        graph capture that contains ``resample``)."""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = torch.from_numpy(np.array(self.taps)).to(device)
        return self._on[device]


@functools.lru_cache(maxsize=None)
def _resample_table(L, M, zeros, rolloff, beta):
    c = rolloff * min(1.0, L / M)
    W = zeros / c
    half = int(math.ceil(W))
    j = np.arange(2 * half, dtype=np.int64)
    r = np.arange(L, dtype=np.int64)[:, None]
    tau = (r + L * (half - 1 - j)) / L                                        # exact integers, one division
    u = tau / W
    with np.errstate(invalid='ignore'):                                      # (sqrt of a negative number where |u| >= 1: selected away)
        window = np.where(np.abs(u) < 1, np.i0(beta * np.sqrt(1 - u * u)) / np.i0(beta), 0.0)
    return ResampleTable(L, M, c * np.sinc(c * tau) * window)


def resample_table(rate_in, rate_out, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF, beta=RESAMPLE_BETA):
    """The ``ResampleTable`` from ``rate_in`` to ``rate_out`` Hz (positive integers), a Kaiser-windowed sinc:
    with g = gcd, L = rate_out/g, M = rate_in/g, c = rolloff min(1, L/M), W = zeros/c, half = ceil(W), T = 2 half,
    tau = (r + L (half - 1 - j)) / L:  taps[r][j] = c sinc(c tau) i0(beta sqrt(1 - (tau/W)^2)) / i0(beta), 0 where |tau| >= W.
    The defaults are resampy's published 'kaiser_best'.  More than 4096 phases or taps (44100 -> 16001: L = 16001) are a ValueError.
    Built once per set of arguments and kept."""
    L, M = _ratio(rate_in, rate_out)
    try:
        zeros, rolloff, beta = float(zeros), float(rolloff), float(beta)
    except (TypeError, ValueError):
        zeros = rolloff = beta = float('nan')
    if not (math.isfinite(zeros) and math.isfinite(rolloff) and math.isfinite(beta) and zeros > 0 and 0 < rolloff <= 1 and beta >= 0):
        raise ValueError('resample_table: zeros > 0, 0 < rolloff <= 1 and beta >= 0 must be finite numbers')
    half = int(math.ceil(zeros / (rolloff * min(1.0, L / M))))
    if L > RESAMPLE_MAX_PHASES or 2 * half > RESAMPLE_MAX_TAPS:
        raise ValueError('resample_table: %r -> %r Hz needs %d phases of %d taps, at most %d and %d are supported'
                         % (rate_in, rate_out, L, 2 * half, RESAMPLE_MAX_PHASES, RESAMPLE_MAX_TAPS))
    return _resample_table(L, M, zeros, rolloff, beta)


def resampled_length(nsamp, rate_in, rate_out):
    """Samples of ``resample`` for ``nsamp`` input samples: ceil(nsamp L / M)."""
    L, M = _ratio(rate_in, rate_out)
    return -(-int(nsamp) * L // M)


def _mix_host(x):
    """numpy ``[nsamp]`` or ``[nsamp, channels]`` -> float32 mono, the bits of the kernels: int16 as v / 32768 (exact), then for more
    than one channel the float32 sum in channel order divided by 2 (dataset.py:287-288)."""
    x = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x.astype(np.float32, copy=False)
    if x.ndim == 1 or x.shape[1] == 1:
        return np.ascontiguousarray(x.reshape(-1))
    acc = np.zeros(x.shape[0], dtype=np.float32)
    for c in range(x.shape[1]):
        acc = acc + x[:, c]
    return acc / np.float32(2)


def _resample_host(m, table, n_out):
    """The numpy twin of csrc/resample.hip on the float32 mono signal ``m``: vectorised over the outputs, a loop over the taps in
    ascending order, fp64 product then fp64 sum (numpy does not fuse), over a zero-padded fp64 copy -- adding the +-0.0 of a term
    outside the signal leaves every bit of the sum as skipping it does (the sum starts at +0.0 and the taps are finite)."""
    L, M, T = table.L, table.M, table.T
    half = T // 2
    p = np.arange(n_out, dtype=np.int64) * M
    q, r = p // L, p % L
    xp = np.zeros(m.shape[0] + T, dtype=np.float64)
    xp[half:half + m.shape[0]] = m
    acc = np.zeros(n_out, dtype=np.float64)
    for j in range(T):
        acc = acc + table.taps[r, j] * xp[q + 1 + j]
    return acc.astype(np.float32)


def resample(signal, rate_in, rate_out, table=None, device='cuda'):
    """Waveform (numpy array or tensor, ``[nsamp]`` or ``[nsamp, channels]``) at ``rate_in`` Hz -> the float32 MONO waveform
    ``[ceil(nsamp L / M)]`` at ``rate_out`` Hz on the device, one launch (pg_resample_mono): mix-down as in ``spectrogram_u8``, then
    out[n] = sum_j taps[r][j] m[q - T/2 + 1 + j] with (q, r) = divmod(n M, L), fp64 in ascending j over the samples that exist, one
    rounding.  int16 samples go to the kernel as they are (v / 32768); every other dtype is converted to float32 on the host.
    ``table``: a ``ResampleTable`` for this L and M (default ``resample_table(rate_in, rate_out)``).  ``device='cpu'``: the numpy twin,
    a numpy array with the same bits.  Equal rates launch nothing and return the mix-down."""
    L, M = _ratio(rate_in, rate_out)
    if table is None:
        table = resample_table(rate_in, rate_out) if L != M else None
    elif not isinstance(table, ResampleTable) or (table.L, table.M) != (L, M):
        raise ValueError('resample: table must be a ResampleTable with L = %d and M = %d, got %r'
                         % (L, M, (table.L, table.M) if isinstance(table, ResampleTable) else type(table).__name__))
    is_tensor = not isinstance(signal, np.ndarray) and hasattr(signal, 'data_ptr')
    if not is_tensor:
        signal = np.asarray(signal)
    if signal.ndim not in (1, 2) or signal.shape[0] < 1 or (signal.ndim == 2 and signal.shape[1] < 1):
        raise ValueError('expected a waveform [nsamp] or [nsamp, channels], got shape %s' % (tuple(signal.shape),))
    nsamp, channels = int(signal.shape[0]), int(signal.shape[1]) if signal.ndim == 2 else 1
    n_out = -(-nsamp * L // M)
    if str(device) == 'cpu':
        m = _mix_host(signal.cpu().numpy() if is_tensor else signal)
        return m if L == M else _resample_host(m, table, n_out)
    import torch
    from . import ops
    if is_tensor:
        t = signal
    else:
        t = torch.from_numpy(np.ascontiguousarray(signal, dtype=np.int16 if signal.dtype == np.int16 else np.float32))
    if t.dtype != torch.int16:
        t = t.to(dtype=torch.float32)
    t = t.to(device=device).contiguous()
    if L == M:                                                                # the mix-down of spectrogram_u8, no launch of ours
        t = t.to(dtype=torch.float32) / 32768 if t.dtype == torch.int16 else t
        return (t.sum(dim=1) / 2 if channels > 1 else t.reshape(-1)).contiguous()
    ops.require_gpu()
    if t.data_ptr() % 16:
        t = t.clone()                                                         # (a slice of a larger tensor: 16-byte aligned bases)
    fmt = _RC['PG_RESAMPLE_I16'] if t.dtype == torch.int16 else _RC['PG_RESAMPLE_F32']
    taps = table.on(t.device)
    out = torch.empty(n_out, device=t.device, dtype=torch.float32)
    with torch.cuda.device(t.device):
        _lib.call('pg_resample_mono', t.data_ptr(), fmt, nsamp, channels, taps.data_ptr(), L, M, table.T, out.data_ptr(), n_out,
                  ops._stream())
    return out


def load_wav(path):
    """``(rate, samples)`` of a WAV file through scipy.io.wavfile.read: ``samples`` is ``[nsamp]`` or ``[nsamp, channels]``, int16 and
    float32 as stored, int32 as float32 v / 2^31, uint8 as float32 (v - 128) / 128.  A file that cannot be read or holds another sample
    type is a ValueError naming it."""
    from scipy.io import wavfile
    try:
        rate, data = wavfile.read(path)
    except Exception as e:
        raise ValueError('%s: cannot be read as a WAV file (%s)' % (path, e))
    data = np.asarray(data)
    if data.dtype in (np.int16, np.float32):
        return int(rate), data
    if data.dtype == np.int32:
        return int(rate), (data / 2147483648.0).astype(np.float32)
    if data.dtype == np.uint8:
        return int(rate), ((data.astype(np.float32) - 128) / 128).astype(np.float32)
    raise ValueError('%s: samples of type %s (int16, float32, int32 and uint8 are supported)' % (path, data.dtype))


def _resample_arguments(rate_in, frequency, img_mode, sample_rate):
    """``(convert, sample_rate)`` of the sound ends' ``rate_in`` / ``frequency`` (the reference's name for the target rate,
    dataset.py:273): both or neither; ``convert`` when they differ; with img_mode='melif' ``sample_rate`` defaults to ``frequency``."""
    if (rate_in is None) != (frequency is None):
        raise ValueError('rate_in and frequency belong together: got rate_in %r and frequency %r' % (rate_in, frequency))
    if frequency is None:
        return False, sample_rate
    L, M = _ratio(rate_in, frequency)
    if img_mode == 'melif':
        if sample_rate is None:
            sample_rate = int(frequency)
        elif sample_rate != frequency:
            raise ValueError("img_mode='melif': sample_rate %r is not the frequency %r the waveform is resampled to" % (sample_rate, frequency))
    return L != M, sample_rate


def _mel_arguments(img_mode, n_fft, sample_rate, mel_rows):
    """The ``phase.MelTable`` of img_mode='melif' (``sample_rate`` defaults to 16000, ``mel_rows`` to n_fft/2), None for every other
    mode -- where ``sample_rate`` and ``mel_rows`` are a ValueError, like ``mag_range``."""
    if img_mode != 'melif':
        if sample_rate is not None or mel_rows is not None:
            raise ValueError("sample_rate and mel_rows belong to img_mode='melif' (got img_mode %r)" % (img_mode,))
        return None
    from . import phase
    if isinstance(n_fft, bool) or int(n_fft) != n_fft:
        raise ValueError('n_fft must be an integer, got %r' % (n_fft,))
    return phase.mel_table(int(n_fft), int(n_fft) // 2 if mel_rows is None else mel_rows, MEL_SAMPLE_RATE if sample_rate is None else sample_rate)


def spectrogram_u8(signal, n_fft=1024, hop_length=128, img_mode='abslog', range_in=(0, 255), mag_range=None, sample_rate=None,
                   mel_rows=None, rate_in=None, frequency=None):
    """Waveform (numpy array or tensor, ``[nsamp]`` or ``[nsamp, channels]``) -> uint8 device image: ``[1, n_fft/2, n_fft/2]``
    for the spectrogram modes 'abslog' (log(1 + |s|), dataset.py:296) and 'reallog' (log(1 + |Re s|) * sign(s), dataset.py:298,
    with numpy 1.13's complex sign = the sign of the real part), ``[1, 2^k, 2^k]`` for 'raw' (the waveform itself, dataset.py:289-291).
    Defaults as SoundImageDataset.__init__ (dataset.py:259-274).

    'magif' (this project's own): ``[2, n_fft/2, n_fft/2]``, log-magnitude stretched from the FIXED ``mag_range``
    (default (0, log1p(n_fft/2))) and the instantaneous frequency on a circle of 256 levels; ``range_in`` is not used.

    'melif' (this project's own): ``[2, M, M]`` with M = ``mel_rows`` (a power of two, 4 <= M <= n_fft/2, default
    n_fft/2) mel-spaced rows made from the n_fft/2 bins at ``sample_rate`` Hz (default 16000), the first M frames; otherwise as 'magif'.

    ``rate_in`` and ``frequency`` (both or neither; SoundImageDataset's ``frequency``, dataset.py:273): the waveform is a recording at
    ``rate_in`` Hz and is brought to ``frequency`` Hz by ``resample`` first; the rest runs on its mono result.  With 'melif'
    ``sample_rate`` then defaults to ``frequency``, and another value is a ValueError."""
    import torch
    from . import ops
    if img_mode not in ('abslog', 'reallog', 'raw', 'magif', 'melif'):
        raise ValueError("img_mode must be one of 'abslog', 'reallog', 'raw', 'magif', 'melif' (got %r)" % (img_mode,))
    if img_mode not in ('magif', 'melif') and mag_range is not None:
        raise ValueError("mag_range belongs to img_mode='magif' and 'melif' (got img_mode %r)" % (img_mode,))
    convert, sample_rate = _resample_arguments(rate_in, frequency, img_mode, sample_rate)
    _mel_arguments(img_mode, n_fft, sample_rate, mel_rows)
    if range_in[0] != 0:
        raise NotImplementedError('range_in must start at 0 (uint8 images)')
    if convert:
        signal = resample(signal, rate_in, frequency)
    t = signal if torch.is_tensor(signal) else torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float32))
    if img_mode in ('magif', 'melif'):
        if t.dim() not in (1, 2) or t.shape[0] < 1:
            raise ValueError('expected a waveform [nsamp] or [nsamp, channels], got shape %s' % (tuple(t.shape),))
        t = t.to(dtype=torch.float32)
        if t.dim() == 2:
            t = t.sum(dim=1) / 2                                              # dataset.py:287-288: s.sum(axis=1) / 2 in float32
        return spectrogram_stack_u8(t[None], n_fft, hop_length, mag_range, img_mode, sample_rate, mel_rows)[0]
    t = t.to(device='cuda', dtype=torch.float32).contiguous()
    return ops.spectrogram_u8(t, int(n_fft), int(hop_length), float(range_in[1]), img_mode=img_mode)


def spectrogram_stack_u8(signals, n_fft=1024, hop_length=128, mag_range=None, img_mode='magif', sample_rate=None, mel_rows=None,
                         rate_in=None, frequency=None):
    """Mono waveforms ``[batch, nsamp]`` (numpy array or tensor) -> uint8 device images ``[batch, 2, n_fft/2, n_fft/2]`` of
    ``img_mode='magif'``, for filling a ``DeviceImageDataset`` stack: the analysis of the whole batch and the quantiser, no host
    synchronisation (phase.spectrogram_stack_u8).  ``img_mode='melif'``: ``[batch, 2, M, M]``, M = ``mel_rows`` mel-spaced rows at
    ``sample_rate`` Hz as in ``spectrogram_u8`` (phase.mel_spectrogram_stack_u8), the same two launches.  ``rate_in`` / ``frequency`` as
    in ``spectrogram_u8``: every row goes through ``resample`` first, one launch per row."""
    import torch
    from . import phase
    if img_mode not in ('magif', 'melif'):
        raise ValueError("img_mode must be 'magif' or 'melif' (got %r)" % (img_mode,))
    convert, sample_rate = _resample_arguments(rate_in, frequency, img_mode, sample_rate)
    t = signals if torch.is_tensor(signals) else torch.from_numpy(np.ascontiguousarray(signals, dtype=np.float32))
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError('signals: expected [batch, nsamp], got shape %s' % (tuple(t.shape),))
    if convert:
        _mel_arguments(img_mode, n_fft, sample_rate, mel_rows)               # (the argument errors before the launches)
        t = torch.stack([resample(row, rate_in, frequency) for row in t])
    if isinstance(n_fft, bool) or int(n_fft) != n_fft or isinstance(hop_length, bool) or int(hop_length) != hop_length:
        raise ValueError('n_fft and hop_length must be integers, got %r and %r' % (n_fft, hop_length))
    table = _mel_arguments(img_mode, n_fft, sample_rate, mel_rows)
    t = t.to(device='cuda', dtype=torch.float32).contiguous()
    if table is not None:
        return phase.mel_spectrogram_stack_u8(t, int(n_fft), int(hop_length), table, mag_range)
    return phase.spectrogram_stack_u8(t, int(n_fft), int(hop_length), mag_range)


def strip_frames(nsamp, hop_length, img_mode='magif'):
    """Columns of ``spectrogram_strip_u8`` for a waveform of ``nsamp`` samples: the 1 + nsamp // hop_length frames without the first."""
    if img_mode not in ('magif', 'abslog', 'melif'):
        raise ValueError("img_mode must be 'magif', 'abslog' or 'melif' (got %r)" % (img_mode,))
    if isinstance(hop_length, bool) or int(hop_length) != hop_length or hop_length < 1:
        raise ValueError('hop_length must be a positive integer, got %r' % (hop_length,))
    return int(nsamp) // int(hop_length)


def spectrogram_strip_u8(signal, n_fft=1024, hop_length=128, img_mode='magif', mag_range=None, sample_rate=None, mel_rows=None,
                         rate_in=None, frequency=None):
    """Waveform (numpy array or tensor, ``[nsamp]`` or ``[nsamp, channels]``, mixed down as in ``spectrogram_u8``) -> the uint8 device
    STRIP ``[C, n_fft/2, T]`` over ALL frames of the recording, T = nsamp // hop_length, for ``dataset.DeviceStripDataset``:
    ``phase.analyse(bins=n_fft/2, frames=all)`` and ``phase.magif_u8`` with column 0 dropped -- the first column of the second
    channel is the phase itself, not an instantaneous frequency, and a crop from the middle of a recording never has such a column.

    'magif'   both channels: log-magnitude stretched from the FIXED ``mag_range`` (default (0, log1p(n_fft/2))) and the instantaneous
              frequency on a circle of 256 levels.
    'abslog'  channel 0 of the same alone, ``[1, n_fft/2, T]``: log1p|S| stretched from the FIXED ``mag_range``, NOT from the per-file
              minimum and maximum that ``spectrogram_u8(img_mode='abslog')`` (the reference's load_file) uses -- crops of one
              recording and of different recordings share one scale, and the image can be inverted without knowing the file.
    'melif'   ``[2, M, T]``: both channels on M = ``mel_rows`` mel-spaced rows at ``sample_rate`` Hz, as in ``spectrogram_u8``
              (``phase.mel_analyse``: the planes of the n_fft/2 linear bins are never written).

    ``rate_in`` / ``frequency`` as in ``spectrogram_u8``: the recording goes through ``resample`` first and T counts the frames of
    its ``resampled_length``.

    The analysis holds two float64 planes [n_fft/2, T + 1] on the device while it runs (16 n_fft/2 bytes per frame)."""
    import torch
    from . import phase
    convert, sample_rate = _resample_arguments(rate_in, frequency, img_mode, sample_rate)
    if convert:
        strip_frames(0, hop_length, img_mode)                                 # (the argument errors before the launch)
        _mel_arguments(img_mode, n_fft, sample_rate, mel_rows)
        signal = resample(signal, rate_in, frequency)
    t = signal if torch.is_tensor(signal) else torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float32))
    if t.dim() not in (1, 2) or t.shape[0] < 1:
        raise ValueError('expected a waveform [nsamp] or [nsamp, channels], got shape %s' % (tuple(t.shape),))
    if isinstance(n_fft, bool) or int(n_fft) != n_fft:
        raise ValueError('n_fft must be an integer, got %r' % (n_fft,))
    T = strip_frames(t.shape[0], hop_length, img_mode)
    table = _mel_arguments(img_mode, n_fft, sample_rate, mel_rows)
    if T < 1:
        raise ValueError('%d samples every %r give no frame after the first' % (t.shape[0], hop_length))
    mag_range = phase.check_mag_range(mag_range, int(n_fft), 'spectrogram_strip_u8')
    t = t.to(device='cuda', dtype=torch.float32)
    if t.dim() == 2:
        t = t.sum(dim=1) / 2                                                  # dataset.py:287-288: s.sum(axis=1) / 2 in float32
    if table is not None:
        logmag, ifreq = phase.mel_analyse(t.contiguous(), int(n_fft), int(hop_length), table, T + 1)
    else:
        logmag, ifreq = phase.analyse(t.contiguous(), int(n_fft), int(hop_length), int(n_fft) // 2, T + 1)
    image = phase.magif_u8(logmag, ifreq, mag_range)[0]
    return image[:1 if img_mode == 'abslog' else 2, :, 1:].contiguous()


# ---------------------------------------------------------------------- 'magif' in numpy fp64: the host twin of csrc/phase.hip
def _mag_range(mag_range, n_fft):
    if mag_range is None:
        return (0.0, float(np.log1p(n_fft // 2)))
    try:
        lo, hi = (float(v) for v in mag_range)
    except (TypeError, ValueError):
        raise ValueError('mag_range must be None or (lo, hi), got %r' % (mag_range,))
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError('mag_range must be finite with hi > lo, got %r' % (mag_range,))
    return (lo, hi)


def magif_analyse(y, n_fft, hop_length):
    """Mono waveform -> ``(logmag, ifreq)`` float64 ``[n_fft/2 + 1, frames]``: log1p(|S|) and the wrapped difference of the phase of
    neighbouring frames in units of pi, in [-1, 1); the first column is the phase itself (phi[-1] = 0, phi = 0 where S == 0)."""
    return _magif_planes(stft(np.asarray(y, dtype=np.float32), n_fft, hop_length))


def _magif_planes(S):
    """``(logmag, ifreq)`` of a complex spectrum ``[bins, frames]``."""
    phi = np.where(np.abs(S) == 0, 0.0, np.arctan2(S.imag, S.real) / np.pi)   # (arctan2(-0.0, -0.0) is -pi)
    d = np.diff(phi, axis=1, prepend=0.0)
    return np.log1p(np.abs(S)), d - 2.0 * np.floor(d / 2.0 + 0.5)


def magif_image(logmag, ifreq, mag_range):
    """Both planes -> uint8 ``[2, ...]``: clip(rint((logmag - lo) / (hi - lo) * 255), 0, 255) and rint((ifreq + 1) * 128) mod 256."""
    lo, hi = mag_range
    m = np.clip(np.rint((np.asarray(logmag, dtype=np.float64) - lo) / (hi - lo) * 255.0), 0, 255)
    f = np.mod(np.rint((np.asarray(ifreq, dtype=np.float64) + 1.0) * 128.0), 256.0)
    return np.stack([m, f]).astype(np.uint8)


def magif_spectrum(image, drange, mag_range):
    """fp32 image ``[2, H, W]`` -> complex spectrum ``[H + 1, W]``: magnitude expm1(max(v, 0)) from channel 0, the running sum of the
    instantaneous frequency of channel 1 as the phase in units of pi; the bin H (Nyquist) is 0."""
    img = np.asarray(image, dtype=np.float64)
    mag = np.expm1(np.maximum(adjust_dynamic_range(img[0], tuple(drange), tuple(mag_range)), 0.0))
    c = np.cumsum(adjust_dynamic_range(img[1], tuple(drange), (0, 255)) / 128.0 - 1.0, axis=1)
    spec = np.zeros((img.shape[1] + 1, img.shape[2]), dtype=np.complex128)
    c = c - 2.0 * np.floor(c / 2.0 + 0.5)                                     # into [-1, 1], exactly: cos / sin see small arguments
    spec[:-1] = mag * (np.cos(np.pi * c) + 1.0j * np.sin(np.pi * c))
    return spec


# ------------------------------------------------------------- 'melif' in numpy fp64: the host twin of csrc/mel.hip (``table``: a
# phase.MelTable, e.g. phase.mel_table(n_fft, rows, sample_rate))
def melif_analyse(y, n_fft, hop_length, table):
    """Mono waveform -> ``(logmag, ifreq)`` float64 ``[table.rows, frames]``: row m is log1p of the weighted mean of |S| over its band
    of bins and the magnitude-weighted circular mean of their instantaneous frequencies (0 where that mean vanishes); a row whose
    band is one bin copies the bin's two values of ``magif_analyse``."""
    if table.n_fft != n_fft:
        raise ValueError('melif_analyse: the table is for n_fft %d, not %d' % (table.n_fft, n_fft))
    S = stft(np.asarray(y, dtype=np.float32), n_fft, hop_length)
    logmag_k, ifreq_k = _magif_planes(S)                                    # (the planes of ``magif_analyse``, from the one transform)
    mag = np.abs(S)
    logmag, ifreq = np.empty((table.rows, S.shape[1])), np.empty((table.rows, S.shape[1]))
    for m in range(table.rows):
        s, n = int(table.start[m]), int(table.count[m])
        if n == 1:
            logmag[m], ifreq[m] = logmag_k[s], ifreq_k[s]
            continue
        a, zr, zi = np.zeros(S.shape[1]), np.zeros(S.shape[1]), np.zeros(S.shape[1])
        for w, k in zip(table.row_weights(m), range(s, s + n)):              # in ascending k, as the kernel sums
            a, zr, zi = a + w * mag[k], zr + w * (mag[k] * np.cos(np.pi * ifreq_k[k])), zi + w * (mag[k] * np.sin(np.pi * ifreq_k[k]))
        logmag[m] = np.log1p(a)
        ifreq[m] = np.where((zr == 0) & (zi == 0), 0.0, np.arctan2(zi, zr) / np.pi)
    return logmag, ifreq


def melif_spectrum(image, table, drange, mag_range):
    """fp32 image ``[2, table.rows, W]`` -> complex spectrum ``[table.bins + 1, W]``: bin k takes its magnitude linearly and its
    instantaneous frequency along the shorter arc between rows lower[k] and lower[k] + 1 (frac 0 / 1: from the one row alone), then
    as ``magif_spectrum``."""
    img = np.asarray(image, dtype=np.float64)
    if img.ndim != 3 or img.shape[:2] != (2, table.rows):
        raise ValueError('melif_spectrum: expected an image [2, %d, W], got shape %s' % (table.rows, tuple(img.shape)))
    a = np.expm1(np.maximum(adjust_dynamic_range(img[0], tuple(drange), tuple(mag_range)), 0.0))
    g = adjust_dynamic_range(img[1], tuple(drange), (0, 255)) / 128.0 - 1.0
    i, f = table.lower.astype(np.int64), table.frac[:, None]
    with np.errstate(invalid='ignore'):                                      # (a non-finite row is selected away below, not multiplied by 0)
        step = g[i + 1] - g[i]
        step = step - 2.0 * np.floor(step / 2.0 + 0.5)
        mag = np.where(f == 0, a[i], np.where(f == 1, a[i + 1], (1.0 - f) * a[i] + f * a[i + 1]))
        d = np.where(f == 0, g[i], np.where(f == 1, g[i + 1], g[i] + f * step))
        c = np.cumsum(d, axis=1)
        spec = np.zeros((table.bins + 1, img.shape[2]), dtype=np.complex128)
        c = c - 2.0 * np.floor(c / 2.0 + 0.5)                                 # into [-1, 1], exactly: cos / sin see small arguments
        spec[:-1] = mag * (np.cos(np.pi * c) + 1.0j * np.sin(np.pi * c))
    return spec


def _frames(y, n_fft, hop):
    """[n_frames, n_fft] view of the reflect-padded signal (frame t starts at t * hop)."""
    yp = np.pad(y, n_fft // 2, mode='reflect')
    n = 1 + (yp.shape[0] - n_fft) // hop
    return np.lib.stride_tricks.as_strided(yp, shape=(n, n_fft), strides=(yp.strides[0] * hop, yp.strides[0]), writeable=False)


def _window(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)        # periodic Hann


def stft(y, n_fft, hop_length):
    """[1 + n_fft/2, n_frames] complex spectrum, all frames in one batched rFFT."""
    return np.fft.rfft(_frames(np.asarray(y, dtype=np.float64), n_fft, hop_length) * _window(n_fft), axis=1).T


def istft(spec, hop_length):
    n_fft = 2 * (spec.shape[0] - 1)
    pieces = np.fft.irfft(spec.T, n_fft, axis=1) * (_window(n_fft) * (2.0 / 3.0))
    y = np.zeros(n_fft + hop_length * (spec.shape[1] - 1))
    for t in range(pieces.shape[0]):                                          # overlap-add
        y[t * hop_length:t * hop_length + n_fft] += pieces[t]
    return y[n_fft // 2:-(n_fft // 2)]


class SoundSaver(object):
    """Post-processor writing generated spectrograms / raw waveforms as WAV files (output_postprocess.py:75-153).  ``mode='magif'``
    (this project's own): channels 0 and 1 are log-magnitude over ``mag_range`` (default (0, log1p(H))) and instantaneous frequency;
    the waveform is ONE inverse STFT of magnitude x e^{i pi cumsum(IF)}, no Griffin-Lim and no random start.  ``mode='melif'``: the
    same for images whose M rows are mel-spaced rows of an ``n_fft``-point transform (default 2 M) at ``sample_rate`` Hz
    (``phase.mel_table``): every one of the n_fft/2 bins is interpolated from its two rows first."""

    output_file_format = 'fakes_sound_{}_{}.wav'

    def __init__(self, samples_path='.', drange=(-1, 1), resolution=512, mode='abslog', sample_rate=16000,
                 hop_length=128, create_subdirs=True, verbose=False, griffin_lim_iter=100, seed=None, mag_range=None, n_fft=None):
        self.samples_path = samples_path
        if mag_range is not None:
            if mode not in ('magif', 'melif'):
                raise ValueError("mag_range belongs to mode='magif' and 'melif' (got mode %r)" % (mode,))
            mag_range = _mag_range(mag_range, 0)
        self.mag_range = mag_range
        if n_fft is not None:
            if mode != 'melif':
                raise ValueError("n_fft belongs to mode='melif' (got mode %r)" % (mode,))
            if isinstance(n_fft, bool) or int(n_fft) != n_fft:
                raise ValueError('n_fft must be an integer, got %r' % (n_fft,))
            n_fft = int(n_fft)
        self.n_fft = n_fft
        if create_subdirs:
            os.makedirs(self.samples_path, exist_ok=True)
        self.drange, self.mode, self.sample_rate, self.hop_length = drange, mode, sample_rate, hop_length
        self.verbose, self.resolution, self.griffin_lim_iter = verbose, resolution, griffin_lim_iter
        self._rng = np.random if seed is None else np.random.RandomState(seed)   # the reference draws from the global numpy RNG

    def reconstruct_from_magnitude(self, stft_mag):
        """Griffin-Lim: keep the given magnitudes, iterate the phases of a random start towards consistency."""
        n_fft = (stft_mag.shape[0] - 1) * 2
        x = self._rng.randn((stft_mag.shape[1] - 1) * self.hop_length)
        for _ in range(self.griffin_lim_iter):
            phase = np.angle(stft(x, n_fft, self.hop_length))
            previous = x
            x = istft(stft_mag * np.exp(1.0j * phase), self.hop_length)
            if self.verbose:
                print('Griffin-Lim: change of the signal in this round (L2) = %g' % np.sqrt(np.square(x - previous).sum()))
        return x

    def mel_table(self, rows):
        """mode='melif': the table between images of ``rows`` rows and the bins of ``self.n_fft`` (default 2 rows) at ``self.sample_rate``."""
        from . import phase
        return phase.mel_table(2 * rows if self.n_fft is None else self.n_fft, rows, self.sample_rate)

    def image_to_sound(self, image):
        if self.mode == 'abslog':
            mag = np.zeros((image.shape[0] + 1, image.shape[1]))               # spectrograms have 2**i + 1 frequency bins
            mag[:image.shape[0], :image.shape[1]] = image
            signal = self.reconstruct_from_magnitude(adjust_dynamic_range(mag, self.drange, (0, 255)))
        elif self.mode == 'reallog':
            signed = np.zeros((image.shape[0] + 1, image.shape[1]))
            signed[:image.shape[0], :image.shape[1]] = image
            signed = adjust_dynamic_range(signed, self.drange, (-1, 1))
            signal = istft((np.exp(np.abs(signed)) - 1) * np.sign(signed), self.hop_length)
        elif self.mode == 'raw':
            signal = image.ravel()
        elif self.mode == 'magif':                                            # image [2, H, W]: one inverse STFT, no random start
            if image.ndim != 3 or image.shape[0] != 2:
                raise ValueError("SoundSaver mode 'magif' takes two-channel images, got shape %s" % (tuple(image.shape),))
            signal = istft(magif_spectrum(image, self.drange, _mag_range(self.mag_range, 2 * image.shape[1])), self.hop_length)
        elif self.mode == 'melif':                                            # image [2, M, W]: the bins from the rows, then as 'magif'
            if image.ndim != 3 or image.shape[0] != 2:
                raise ValueError("SoundSaver mode 'melif' takes two-channel images, got shape %s" % (tuple(image.shape),))
            table = self.mel_table(image.shape[1])
            signal = istft(melif_spectrum(image, table, self.drange, _mag_range(self.mag_range, table.n_fft)), self.hop_length)
        else:
            raise ValueError('SoundSaver mode %r is not one of abslog / reallog / raw / magif / melif' % (self.mode,))
        return signal / np.abs(signal).max()

    def output_wav(self, signal, samples_description, ith):
        from scipy.io import wavfile
        fname = self.output_file_format
        fname = fname.format('{:06}' if type(samples_description) is int else '{}', '{:02}')
        try:
            wav = np.asarray(signal, dtype=np.float64)
            wav = (wav / np.abs(wav).max()).astype(np.float32)                # librosa.output.write_wav(..., norm=True)
            wavfile.write(os.path.join(self.samples_path, fname.format(samples_description, ith)), self.sample_rate, wav)
        except Exception as e:
            with open(os.path.join(self.samples_path, 'error_{}_{}.txt'.format(samples_description, ith)), 'w') as f:
                f.write('writing the WAV file failed: %r' % (e,))

    def __call__(self, output, samples_description):
        output = np.asarray(output.cpu().numpy() if hasattr(output, 'cpu') else output)
        times_smaller = self.resolution // output.shape[-1]
        if self.mode == 'raw':
            times_smaller *= times_smaller
        for i, img in enumerate(output):
            signal = self.image_to_sound(img[:2] if self.mode in ('magif', 'melif') else img[0])
            if times_smaller > 1:
                signal = signal.repeat(times_smaller, axis=-1)                # utils.numpy_upsample_nearest(signal, 1, scale_factor=...)
            self.output_wav(signal, samples_description, i)


def _to_device(t):
    return t.cuda()


class DeviceSoundSaver(SoundSaver):
    """``SoundSaver`` with the arithmetic on the device (csrc/griffinlim.hip): same constructor, ``seed``, file names and WAV writer.
    ``plugins.OutputGenerator`` and ``utils.output_samples`` hand it G's device tensor (``accepts_device_tensors``); the samples of
    one call are transformed as one batch, and only their float32 waveforms cross to the host.  The random starts of Griffin-Lim are
    drawn on the HOST from the object's RNG -- one ``randn((W - 1) * hop_length)`` per sample in sample order, exactly the draws
    ``SoundSaver`` makes -- and uploaded once, so ``seed=`` gives the same WAVs from both savers (``metrics.SlicedWasserstein``
    treats its randomness the same way).  Images must be square with a power-of-two side in 4 .. 1024; there is no fallback to the
    host.  ``verbose=True`` prints the host saver's line per round and sample; it copies both signals back after every round, a slow
    debugging aid.  ``mode='magif'`` takes ``[n, 2, H, W]`` samples (further channels are ignored) through csrc/phase.hip: spectrum, pieces,
    overlap-add and normalisation, four launches, and draws nothing from the RNG.  ``mode='melif'`` is the same through csrc/mel.hip's
    spectrum (``phase.mel_synthesise``): four launches as well."""

    accepts_device_tensors = True            # plugins.OutputGenerator then skips the D2H copy of the fp32 samples

    def to_waveforms(self, output):
        """fp32 ``[n, 1, H, W]`` samples (device tensor, or numpy array / host tensor, which is uploaded) -> float32 device tensor
        ``[n, nsamp * times_smaller]``: each sample's waveform, peak-normalised and stretched as ``SoundSaver.__call__`` writes it."""
        import torch
        from . import ops
        if self.mode not in ('abslog', 'reallog', 'raw', 'magif', 'melif'):
            raise ValueError('SoundSaver mode %r is not one of abslog / reallog / raw / magif / melif' % (self.mode,))
        two = self.mode in ('magif', 'melif')
        t = output if torch.is_tensor(output) else torch.from_numpy(np.ascontiguousarray(output, dtype=np.float32))
        if t.dim() != 4 or t.shape[0] < 1 or (two and t.shape[1] < 2):
            raise ValueError('DeviceSoundSaver: expected samples [n, %d, H, W], got shape %s' % (2 if two else 1, tuple(t.shape)))
        n, _, H, W = t.shape
        if H != W or H < 4 or H > 1024 or H & (H - 1):
            raise ValueError('DeviceSoundSaver: images must be square with a power-of-two side in 4 .. 1024, got %dx%d' % (H, W))
        times_smaller = self.resolution // W
        if self.mode == 'raw':
            times_smaller *= times_smaller
        nsamp = (W - 1) * self.hop_length
        table = self.mel_table(H) if self.mode == 'melif' else None
        pad = H if table is None else table.bins
        if self.mode != 'raw' and nsamp <= pad:
            raise ValueError('DeviceSoundSaver: %d frames every %d samples give %d samples, the reflect padding by n_fft/2 = %d '
                             'needs more' % (W, self.hop_length, nsamp, pad))
        if table is not None:                                                 # as 'magif' below, the spectrum from csrc/mel.hip
            from . import phase
            x = phase.mel_synthesise(_to_device(t)[:, :2].to(torch.float32).contiguous(), self.hop_length, table, self.drange, self.mag_range)
            return ops.wave_normalize(x, max(1, times_smaller))
        if self.mode == 'magif':                                              # spectrum, pieces, overlap-add, normalise: four launches,
            from . import phase                                               # no random draws (the RNG is not advanced)
            x = phase.synthesise(_to_device(t)[:, :2].to(torch.float32).contiguous(), self.hop_length, self.drange, self.mag_range)
            return ops.wave_normalize(x, max(1, times_smaller))
        img = _to_device(t)[:, 0].to(torch.float32).contiguous()             # channel 0, as image_to_sound(img[0])
        if self.mode == 'raw':
            x = img.reshape(n, H * W).to(torch.float64)                       # image.ravel(): a cast, the arithmetic is the kernel's
        else:
            x0, hook = None, None
            if self.mode == 'abslog':
                x0 = _to_device(torch.from_numpy(np.stack([self._rng.randn(nsamp) for _ in range(n)])))
                hook = self._print_round if self.verbose else None
            x = ops.griffin_lim(img, x0, self.hop_length, self.griffin_lim_iter, self.mode, self.drange, round_hook=hook)
        return ops.wave_normalize(x, max(1, times_smaller))

    @staticmethod
    def _print_round(i, previous, x):
        for a, b in zip(x.cpu().numpy(), previous.cpu().numpy()):
            print('Griffin-Lim: change of the signal in this round (L2) = %g' % np.sqrt(np.square(a - b).sum()))

    def __call__(self, output, samples_description):
        for i, wav in enumerate(self.to_waveforms(output).cpu().numpy()):
            self.output_wav(wav, samples_description, i)                      # (its own normalisation is the identity: the peak is 1)
