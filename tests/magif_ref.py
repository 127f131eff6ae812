"""TEST INFRASTRUCTURE: the magnitude + instantaneous-frequency definitions (include/pggan_hip_phase.h) in numpy
fp64, built on ``oracle.sound_steps.stft`` / ``istft`` (imported, not edited).  This is the reference the kernels of csrc/phase.hip
and both ``SoundSaver``s are held against; it shares no code with the product (``sound.magif_*`` is written on sound.py's own batched
transforms, this file on the oracle's per-frame loops)."""
import numpy as np

from oracle import sound_steps as oss


def signal(ns, seed):
    """"The test signal": a chirp at half scale plus noise, clipped to [-1, 1], float32."""
    t = np.arange(ns)
    y = 0.5 * np.sin(2 * np.pi * (0.01 * t + 0.2 * t * t / (2.0 * ns))) + 0.1 * np.random.RandomState(seed).randn(ns)
    return np.clip(y, -1, 1).astype(np.float32)


def wrap(d):
    return d - 2.0 * np.floor(d / 2.0 + 0.5)


def default_mag_range(n_fft):
    return (0.0, float(np.log1p(n_fft // 2)))


def analyse(y, n_fft, hop):
    """fp32 waveform -> (S, logmag, ifreq), each [n_fft/2 + 1, 1 + nsamp // hop]."""
    S = oss.stft(np.asarray(y, dtype=np.float32).astype(np.float64), n_fft, hop)
    mag = np.abs(S)
    phi = np.where(mag == 0, 0.0, np.arctan2(S.imag, S.real) / np.pi)
    prev = np.concatenate([np.zeros((phi.shape[0], 1)), phi[:, :-1]], axis=1)
    return S, np.log1p(mag), wrap(phi - prev)


def quantise(logmag, ifreq, mag_range):
    """-> uint8 [2, ...]."""
    lo, hi = mag_range
    ch0 = np.clip(np.rint((logmag - lo) / (hi - lo) * 255), 0, 255)
    ch1 = np.rint((ifreq + 1) * 128) % 256
    return np.stack([ch0, ch1]).astype(np.uint8)


def image(y, n_fft, hop, mag_range=None):
    """img_mode='magif': uint8 [2, n_fft/2, n_fft/2]."""
    _, logmag, ifreq = analyse(y, n_fft, hop)
    h = n_fft // 2
    return quantise(logmag[:h, :h], ifreq[:h, :h], default_mag_range(n_fft) if mag_range is None else mag_range)


def running_sum(img, drange):
    """fp32 [2, H, W] -> (ifreq, c) [H, W]."""
    q = oss.adjust_dynamic_range(np.asarray(img[1], dtype=np.float64), tuple(drange), (0, 255))
    ifreq = q / 128 - 1
    return ifreq, np.cumsum(ifreq, axis=1)


def spectrum(img, drange=(-1, 1), mag_range=None):
    """fp32 [2, H, W] -> complex [H + 1, W]."""
    H, W = img.shape[1:]
    mag_range = default_mag_range(2 * H) if mag_range is None else mag_range
    v = oss.adjust_dynamic_range(np.asarray(img[0], dtype=np.float64), tuple(drange), tuple(mag_range))
    mag = np.expm1(np.maximum(v, 0))
    _, c = running_sum(img, drange)
    r = wrap(c)                                                            # exact: c - (an even integer), no larger than c
    spec = np.zeros((H + 1, W), dtype=np.complex128)
    spec[:H] = mag * (np.cos(np.pi * r) + 1j * np.sin(np.pi * r))
    return spec


def pieces(spec):
    """complex [n_fft/2 + 1, W] -> [W, n_fft]: the summands of oss.istft."""
    n_fft = 2 * (spec.shape[0] - 1)
    win = oss.hann_periodic(n_fft) * (2.0 / 3.0)
    return np.stack([win * np.fft.irfft(spec[:, t], n_fft) for t in range(spec.shape[1])])


def synthesise(img, hop, drange=(-1, 1), mag_range=None):
    return oss.istft(spectrum(img, drange, mag_range), hop)


def from_planes(logmag, ifreq, hop):
    """The inverse of ``analyse`` on unquantised planes with all n_fft/2 + 1 bins."""
    r = wrap(np.cumsum(ifreq, axis=1))
    return oss.istft(np.expm1(logmag) * (np.cos(np.pi * r) + 1j * np.sin(np.pi * r)), hop)
