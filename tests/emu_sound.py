"""Contracts of the four entry points of csrc/griffinlim.hip for the CPU tier (test infrastructure, installed over the ``ops`` wrappers by
tests/test_griffinlim_host.py): numpy fp64 on host tensors, written from include/pggan_hip.h and not from the kernels -- the transforms
are ``np.fft``'s.  The wrappers' own argument checks are for device tensors and are exercised on the device (tests/test_griffinlim_gpu.py)."""
import numpy as np
import torch


def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def gl_spectrum(images, mode='abslog', drange=(-1, 1)):
    """pg_gl_spectrum_f64: pad with a zero row, THEN adjust the range; [n, W, H + 1]."""
    img = images.numpy().astype(np.float64)
    if img.ndim == 4:
        img = img[:, 0]
    n, H, W = img.shape
    v = np.zeros((n, H + 1, W))
    v[:, :H] = img
    range_out = (0, 255) if mode == 'abslog' else (-1, 1)
    if tuple(drange) != range_out:
        v = (v - drange[0]) * ((range_out[1] - range_out[0]) / (drange[1] - drange[0])) + range_out[0]
    if mode == 'reallog':
        v = (np.exp(np.abs(v)) - 1) * np.sign(v)
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 1)))


def gl_pieces(x, spec, hop, out=None):
    """pg_gl_pieces_f64: frame, window, FFT, keep spec's magnitude and the frame's phase (S == 0: phase factor 1), irfft, window * 2/3."""
    sp = spec.numpy()
    batch, frames, bins = sp.shape
    n_fft = 2 * (bins - 1)
    win = hann(n_fft)
    full = sp.astype(np.complex128)
    if x is not None:
        xs = x.numpy()
        assert xs.shape == (batch, hop * (frames - 1)) and xs.shape[1] > n_fft // 2
        for b in range(batch):
            yp = np.pad(xs[b], n_fft // 2, mode='reflect')
            for t in range(frames):
                S = np.fft.rfft(win * yp[t * hop:t * hop + n_fft])
                mod = np.abs(S)
                unit = np.where(mod > 0, S / np.where(mod > 0, mod, 1.0), 1.0)
                full[b, t] = sp[b, t] * unit
    pieces = np.fft.irfft(full, n_fft, axis=2) * (win * (2.0 / 3.0))
    res = torch.from_numpy(pieces)
    if out is not None:
        out.copy_(res)
        return out
    return res


def overlap_add(pieces, hop, out=None):
    """pg_overlap_add_f64: frames added in ascending order from 0.0, the centring pad cut off."""
    pc = pieces.numpy()
    batch, frames, n_fft = pc.shape
    y = np.zeros((batch, n_fft + hop * (frames - 1)))
    for t in range(frames):
        y[:, t * hop:t * hop + n_fft] += pc[:, t]
    res = torch.from_numpy(np.ascontiguousarray(y[:, n_fft // 2:n_fft // 2 + hop * (frames - 1)]))
    if out is not None:
        out.copy_(res)
        return out
    return res


def wave_normalize(x, repeat=1):
    """pg_wave_normalize_f32: fp64 division by the peak, float32 rounding, nearest repeat."""
    xs = x.numpy()
    return torch.from_numpy((xs / np.abs(xs).max(axis=1, keepdims=True)).repeat(repeat, axis=1).astype(np.float32))
