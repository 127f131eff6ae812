"""TEST REFERENCE: the definition of the loss and weight statistics (include/pggan_hip.h "Statistics of the training
process") restated in plain numpy fp64, independent of the product's twin (pggan-pytorch_amd/telemetry.py) and of the kernels.

Sums are taken with ``math.fsum`` -- exactly rounded -- so the reference's own error is half a unit in the last place and the bounds
below measure the code under test alone.  The bounds are the worst case of ANY order of summation (Higham, Accuracy and Stability of
Numerical Algorithms, §4.2: n - 1 additions, each with relative error <= u = 2^-53, give |error| <= (n - 1) u sum|x_i| to first order;
n u covers the second-order terms for every n used here and the one rounding of the reference):

    sum     |got - ref| <= n u sum|x|
    sumsq   |got - ref| <= n u ref            (every term (double)x * (double)x is exact: 24-bit x 24-bit significands)
    mean    |got - ref| <= (n + 1) u sum|x| / n          (the division rounds once more)
"""
import math

import numpy as np

U = 2.0 ** -53
RECORD_FIELDS = ('n_finite', 'sum', 'sumsq', 'min', 'max', 'last', 'n_nonfinite', 'first_bad')
EMPTY = (0.0, 0.0, 0.0, float('inf'), float('-inf'), float('nan'), 0.0, -1.0)


def source_value(x):
    """The value of a source: the mean of its elements in fp64 (NaN / +-Inf when any element is; math.fsum refuses those)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if not np.isfinite(x).all():
        with np.errstate(all='ignore'):
            return float(np.sum(x) / x.size)
    return math.fsum(x.tolist()) / x.size


def value_bound(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return (x.size + 1) * U * math.fsum(np.abs(x).tolist()) / x.size


def fold(record, value):
    """One push of one slot: ``record`` is a list of the eight fields, folded in place, push by push, in fp64 (this order IS the
    definition: a record is a running one)."""
    if math.isfinite(value):
        record[0] += 1.0
        record[1] += value
        record[2] += value * value
        record[3] = min(record[3], value)
        record[4] = max(record[4], value)
    else:
        if record[7] < 0:
            record[7] = record[0] + record[6]
        record[6] += 1.0
    record[5] = value
    return record


def summary(record):
    n = record[0]
    if n == 0:
        mean = std = float('nan')
    else:
        mean = record[1] / n
        std = math.sqrt(max(record[2] / n - mean * mean, 0.0))
    return dict(mean=mean, std=std, min=record[3], max=record[4], last=record[5], count=int(n), nonfinite=int(record[6]),
                first_bad=int(record[7]))


def segment_stats(flat, segments):
    """[S, 4] float64: sum, sumsq, maxabs, n_nonfinite over the finite elements of every (offset, length) segment of ``flat`` (fp32)."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    out = np.zeros((len(segments), 4))
    for s, (off, n) in enumerate(segments):
        x = flat[off:off + n]
        assert x.size == n
        ok = np.isfinite(x)
        d = x[ok].astype(np.float64)
        out[s] = (math.fsum(d.tolist()), math.fsum((d * d).tolist()), float(np.abs(d).max()) if d.size else 0.0, float(n - d.size))
    return out


def segment_bounds(flat, segments):
    """[S, 2]: the bounds on |sum| and |sumsq| errors of every segment, from the header of this file."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    out = np.zeros((len(segments), 2))
    for s, (off, n) in enumerate(segments):
        x = flat[off:off + n]
        d = x[np.isfinite(x)].astype(np.float64)
        out[s] = (n * U * math.fsum(np.abs(d).tolist()), n * U * math.fsum((d * d).tolist()))
    return out


CHUNK = 8192
LENGTHS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 20000)      # every path of the chunk kernel: tail only, one group, group + tail,
#                                                                    a chunk less one, exactly one, one more, several with a ragged last


def layout(count):
    """``count`` segments cycling through LENGTHS in one buffer, each at a multiple of 4 elements with 4 .. 7 floats of padding behind
    it (the networks' layout pads to the next multiple of 4; one more group here, so that every segment has padding on both sides).
    Returns (segments, total floats)."""
    segments, off = [], 4
    for i in range(count):
        n = LENGTHS[i % len(LENGTHS)]
        segments.append((off, n))
        off += (n + 3) // 4 * 4 + 4
    return segments, off


def fill(total, segments, kind, seed=0):
    """A float32 buffer: NaN in the padding (it belongs to no segment and must never reach a result), the segments filled with
    integers of [-1024, 1024] ('int': every sum is exact in fp64) or standard normal draws ('randn')."""
    rng = np.random.RandomState(seed)
    flat = np.full(total, np.nan, dtype=np.float32)
    for off, n in segments:
        flat[off:off + n] = rng.randint(-1024, 1025, size=n) if kind == 'int' else rng.standard_normal(n)
    return flat
