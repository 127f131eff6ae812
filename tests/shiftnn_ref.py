"""TEST INFRASTRUCTURE: the shift-invariant window search of csrc/shift_search.hip / metrics.ShiftNearestNeighbours stated by brute
force in numpy int64: every window of every strip is materialised (``sliding_window_view``) and compared with every query.  It
shares no code with the product's numpy twin (metrics._shift_keys_host), which never materialises a window.

    d[k, m, u]  = sum_{c,r,j} (strip_m[c, r, u + j] - q_k[c, r, j])^2
    key[k, g]   = min over the starts u of segment g of  d * 2^POS_BITS + (u - first start of g)

POS_BITS is stated here, not imported: the header's value is held against it by the tests."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

POS_BITS = 16


def strips(cols, C, S, seed):
    """Random uint8 strips [C,S,T] that use the whole byte range, 0 and 255 included."""
    rng = np.random.RandomState(seed)
    out = []
    for T in cols:
        s = rng.randint(0, 256, size=(C, S, T)).astype(np.uint8)
        s.reshape(-1)[:2] = (0, 255)
        out.append(s)
    return out


def queries(K, C, S, seed):
    rng = np.random.RandomState(seed)
    q = rng.randint(0, 256, size=(K, C, S, S)).astype(np.uint8)
    q.reshape(-1)[:2] = (255, 0)
    return q


def distances(strip, q):
    """int64 [K, T - S + 1]: every query against every window of one strip."""
    S = strip.shape[1]
    win = sliding_window_view(strip, S, axis=2)                              # [C, S, n, S(j)]
    win = np.ascontiguousarray(win.transpose(2, 0, 1, 3)).astype(np.int64)   # [n, C, S, S]
    out = np.empty((q.shape[0], win.shape[0]), dtype=np.int64)
    for k in range(q.shape[0]):
        diff = win - q[k].astype(np.int64)[None]
        out[k] = (diff * diff).reshape(win.shape[0], -1).sum(axis=1)
    return out


def segments(cols, S, seg):
    """[(strip, first start, number of starts)] strip-major."""
    out = []
    for m, T in enumerate(cols):
        n = T - S + 1
        for g0 in range(0, n, seg):
            out.append((m, g0, min(seg, n - g0)))
    return out


def keys(strip_list, q, seg):
    """int64 [K, G]."""
    S = strip_list[0].shape[1]
    dist = [distances(s, q) for s in strip_list]
    cols = []
    for m, g0, n in segments([s.shape[2] for s in strip_list], S, seg):
        best = None
        for u in range(g0, g0 + n):                                          # explicit: (distance, start) ascending, ties to the lower start
            cand = dist[m][:, u] * (1 << POS_BITS) + (u - g0)
            best = cand if best is None else np.minimum(best, cand)
        cols.append(best)
    return np.stack(cols, axis=1)


def search(strip_list, q, seg, k):
    """(strip [K,k], start [K,k], sqdist [K,k]) ascending by (sqdist, start within the segment, segment)."""
    S = strip_list[0].shape[1]
    segs = segments([s.shape[2] for s in strip_list], S, seg)
    key = keys(strip_list, q, seg)
    order = np.stack([np.lexsort((np.arange(row.size), row))[:k] for row in key])
    val = np.take_along_axis(key, order, axis=1)
    strip = np.array([[segs[g][0] for g in row] for row in order], dtype=np.int64)
    first = np.array([[segs[g][1] for g in row] for row in order], dtype=np.int64)
    return strip, first + (val & ((1 << POS_BITS) - 1)), val >> POS_BITS
