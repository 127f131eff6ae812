"""TEST INFRASTRUCTURE: the rate conversion of include/pggan_hip_resample.h restated independently of
pggan-pytorch_amd/sound.py: the table from the formula one tap at a time, a direct double loop for the outputs (tiny inputs only),
the vectorised form of the same sum, and seeded test signals.  numpy float64; nothing here imports the package."""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492           # resampy's published 'kaiser_best'


def ratio(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g                                       # L, M


def length(nsamp, rate_in, rate_out):
    L, M = ratio(rate_in, rate_out)
    return (nsamp * L + M - 1) // M


def table(rate_in, rate_out, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """float64 [L, T] from the formula, one phase row at a time (np.sinc and np.i0 are the definition's functions; the window is
    evaluated only where |u| < 1)."""
    L, M = ratio(rate_in, rate_out)
    c = rolloff * min(1.0, L / M)
    W = zeros / c
    half = int(math.ceil(W))
    T = 2 * half
    taps = np.zeros((L, T))
    i0b = np.i0(beta)
    j = np.arange(T)
    for r in range(L):
        tau = (r + L * (half - 1 - j)) / L
        u = tau / W
        inside = np.abs(u) < 1
        win = np.zeros(T)
        win[inside] = np.i0(beta * np.sqrt(1 - u[inside] * u[inside])) / i0b
        taps[r] = c * np.sinc(c * tau) * win
    return taps


def mix(x):
    """float32 mono of [nsamp] or [nsamp, channels] (float32 or int16): int16 is v / 32768 first; more than one channel is the float32
    sum in channel order divided by 2."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        x = (x.astype(np.float64) / 32768.0).astype(np.float32)             # (exact in either precision)
    assert x.dtype == np.float32
    if x.ndim == 1:
        return x
    if x.shape[1] == 1:
        return x[:, 0]
    acc = np.float32(0)
    for c in range(x.shape[1]):
        acc = (acc + x[:, c]).astype(np.float32)
    return (acc / np.float32(2)).astype(np.float32)


def direct(m, taps, L, M):
    """The definition as it is written: one output and one tap at a time, terms outside the signal skipped."""
    m = np.asarray(m, dtype=np.float32)
    nsamp, T = m.shape[0], taps.shape[1]
    half = T // 2
    n_out = (nsamp * L + M - 1) // M
    out = np.zeros(n_out, dtype=np.float32)
    for n in range(n_out):
        q, r = divmod(n * M, L)
        acc = 0.0
        for j in range(T):
            k = q - half + 1 + j
            if 0 <= k < nsamp:
                acc = acc + float(taps[r, j]) * float(m[k])
        out[n] = np.float32(acc)
    return out


def vectorised(m, taps, L, M):
    """The same sum for all outputs at once, tap after tap in ascending order, with an explicit mask instead of padding."""
    m = np.asarray(m, dtype=np.float32).astype(np.float64)
    nsamp, T = m.shape[0], taps.shape[1]
    half = T // 2
    n_out = (nsamp * L + M - 1) // M
    p = np.arange(n_out, dtype=np.int64) * M
    q, r = p // L, p % L
    acc = np.zeros(n_out)
    for j in range(T):
        k = q - half + 1 + j
        ok = (k >= 0) & (k < nsamp)
        term = taps[r, j] * m[np.clip(k, 0, nsamp - 1)]
        acc = np.where(ok, acc + term, acc)
    return acc.astype(np.float32)


def signal(nsamp, seed, channels=1, dtype=np.float32):
    """Seeded noise in [-1, 1): float32, or int16 over the whole range; [nsamp] for one channel, else [nsamp, channels]."""
    rs = np.random.RandomState(seed)
    shape = (nsamp,) if channels == 1 else (nsamp, channels)
    if dtype == np.int16:
        return rs.randint(-32768, 32768, size=shape).astype(np.int16)
    return (rs.rand(*shape) * 2 - 1).astype(np.float32)


def sine(nsamp, freq, rate):
    """float32 sine of ``freq`` Hz sampled at ``rate`` Hz, and the function of time (seconds) it samples."""
    f = lambda t: np.sin(2.0 * np.pi * freq * t)
    return f(np.arange(nsamp) / rate).astype(np.float32), f
