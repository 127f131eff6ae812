"""TEST INFRASTRUCTURE: the 'melif' definitions (include/pggan_hip_mel.h) in numpy fp64, built on
``oracle.sound_steps.stft`` / ``istft`` and on tests/magif_ref.py (both imported, not edited).  This is the reference the kernels of
csrc/mel.hip, ``sound.melif_*`` and both ``SoundSaver``s are held against.  It imports neither sound.py nor phase.py and is written
another way: the warp is a DENSE matrix ``[M, H]`` applied with matrix products, the table's formulas are restated per element.

A table here is a ``Table``: the dense weights ``W [M, H]`` plus ``lower`` / ``frac`` [H]; ``arrays()`` gives the sparse form that
``phase.MelTable`` takes, so that a test can hand the product the reference's own table."""
import collections
import functools
import math

import numpy as np

import magif_ref as mref
from oracle import sound_steps as oss

signal, wrap, default_mag_range = mref.signal, mref.wrap, mref.default_mag_range

# the (M, H, sr) of the issue's list: M = H at every size, the oversampled ones, and two at 44.1 kHz
TABLES = [(M, M, 16000) for M in (4, 8, 16, 32, 64, 128, 256, 512, 1024)] + \
         [(4, 16, 16000), (64, 256, 16000), (128, 1024, 16000), (256, 1024, 16000), (512, 1024, 16000), (512, 512, 44100), (256, 1024, 44100)]


class Table(collections.namedtuple('Table', 'n_fft rows W lower frac p q')):
    @property
    def bins(self):
        return self.n_fft // 2

    def arrays(self):
        """(start, count, flat weights, lower, frac): every row's contiguous band of non-zero weights."""
        start, count, weights = [], [], []
        for row in self.W:
            nz = np.flatnonzero(row)
            assert len(nz) and np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))
            start.append(int(nz[0]))
            count.append(len(nz))
            weights.append(row[nz])
        return np.array(start), np.array(count), np.concatenate(weights), self.lower.copy(), self.frac.copy()


def mel(f):
    return 1127.0 * math.log1p(f / 700.0)


def mel_inv(m):
    return 700.0 * math.expm1(m / 1127.0)


@functools.lru_cache(maxsize=None)
def table(n_fft, rows, sr=16000):
    """The mel table (kept: treat its arrays as read-only)."""
    H, M = n_fft // 2, rows
    top = mel((H - 1) * sr / n_fft)
    p = [mel_inv(m * top / (M - 1)) * n_fft / sr for m in range(M)]
    p[0], p[M - 1] = 0.0, float(H - 1)
    W = np.zeros((M, H))
    for m in range(M):
        l = max(p[m] - p[m - 1], 1.0) if m > 0 else max(p[1] - p[0], 1.0)
        r = max(p[m + 1] - p[m], 1.0) if m < M - 1 else max(p[M - 1] - p[M - 2], 1.0)
        d = np.arange(H) - p[m]
        W[m] = np.where(d <= 0, np.maximum(0.0, 1.0 + d / l), np.maximum(0.0, 1.0 - d / r))
        W[m] = W[m] / W[m].sum()
    q = [mel(k * sr / n_fft) / top * (M - 1) for k in range(H)]
    q[0], q[H - 1] = 0.0, float(M - 1)
    lower = np.array([min(math.floor(v), M - 2) for v in q], dtype=np.int64)
    return Table(n_fft, M, W, lower, np.array(q) - lower, np.array(p), np.array(q))


def identity(n_fft):
    """M = H, row m is bin m.  The last bin sits on the last row as frac 1 above row M - 2 (lower stays within [0, M - 2])."""
    H = n_fft // 2
    frac = np.zeros(H)
    frac[-1] = 1.0
    return Table(n_fft, H, np.eye(H), np.minimum(np.arange(H), H - 2), frac, np.arange(H, dtype=float), np.arange(H, dtype=float))


def analyse(y, n_fft, hop, tab):
    """fp32 waveform -> (a, logmag, ifreq, z): the mean magnitude, both mel planes and the circular mean z, each [M, 1 + nsamp // hop]."""
    S, logmag_k, ifreq_k = mref.analyse(y, n_fft, hop)
    H = n_fft // 2
    mag, fr = np.abs(S[:H]), ifreq_k[:H]
    a = tab.W @ mag
    z = tab.W @ (mag * np.cos(np.pi * fr)) + 1j * (tab.W @ (mag * np.sin(np.pi * fr)))
    g = np.where(z == 0, 0.0, np.arctan2(z.imag, z.real) / np.pi)
    logmag = np.log1p(a)
    for m in range(tab.rows):                                              # a one-bin row copies the bin
        nz = np.flatnonzero(tab.W[m])
        if len(nz) == 1:
            k = int(nz[0])
            a[m], logmag[m], g[m], z[m] = mag[k], logmag_k[k], fr[k], S[k]         # (|z| = |S|: the weight of that row's IF)
    return a, logmag, g, z


def image(y, n_fft, hop, tab, mag_range=None, frames=None):
    """uint8 [2, M, frames] (default: the first M frames) and the two values BEFORE rint, for the half-integer rule."""
    _, logmag, g, _ = analyse(y, n_fft, hop, tab)
    frames = tab.rows if frames is None else frames
    lo, hi = default_mag_range(n_fft) if mag_range is None else mag_range
    before = np.stack([(logmag[:, :frames] - lo) / (hi - lo) * 255, (g[:, :frames] + 1) * 128])
    return mref.quantise(logmag[:, :frames], g[:, :frames], (lo, hi)), before


def rows_to_bins(img, tab, drange=(-1, 1), mag_range=None):
    """fp32 [2, M, W] -> (mag, d) [H, W] of the linear bins."""
    mag_range = default_mag_range(tab.n_fft) if mag_range is None else mag_range
    v = oss.adjust_dynamic_range(np.asarray(img[0], dtype=np.float64), tuple(drange), tuple(mag_range))
    a = np.expm1(np.maximum(v, 0))
    g = oss.adjust_dynamic_range(np.asarray(img[1], dtype=np.float64), tuple(drange), (0, 255)) / 128 - 1
    mag, d = np.empty((tab.bins, a.shape[1])), np.empty((tab.bins, a.shape[1]))
    for k in range(tab.bins):
        i, f = int(tab.lower[k]), float(tab.frac[k])
        if f == 0.0:                                                       # reads row i alone
            mag[k], d[k] = a[i], g[i]
        elif f == 1.0:                                                     # ... and row i + 1 alone
            mag[k], d[k] = a[i + 1], g[i + 1]
        else:
            mag[k] = (1 - f) * a[i] + f * a[i + 1]
            d[k] = g[i] + f * wrap(g[i + 1] - g[i])
    return mag, d


def spectrum(img, tab, drange=(-1, 1), mag_range=None):
    """fp32 [2, M, W] -> (complex [H + 1, W], c [H, W])."""
    mag, d = rows_to_bins(img, tab, drange, mag_range)
    c = np.cumsum(d, axis=1)
    r = wrap(c)
    spec = np.zeros((tab.bins + 1, mag.shape[1]), dtype=np.complex128)
    spec[:-1] = mag * (np.cos(np.pi * r) + 1j * np.sin(np.pi * r))
    return spec, c


def synthesise(img, hop, tab, drange=(-1, 1), mag_range=None):
    return oss.istft(spectrum(img, tab, drange, mag_range)[0], hop)
