"""TEST INFRASTRUCTURE: precision / recall / density / coverage over k-NN balls (csrc/prd.hip, metrics.PrecisionRecall) stated in numpy
int64, written from the definition and not from the kernels.  Exact integer arithmetic: the tests compare with ``==``.

Images are uint8 vectors of D bytes, d2(x, y) = sum_d (x_d - y_d)^2 in int64.
  radius     rad_k(X)[i] = the k-th smallest of { d2(X[i], X[j]) : j != i } -- the exclusion is by INDEX: a duplicate of image i at
             another index counts, with distance 0.  N >= k + 1.
  inside     probe p is inside the ball of centre c iff d2(p, c) <= rad[c] (the boundary is inside).
With fakes G (the probes a of ``ball_counts``) and reals R (b):
  precision  the fraction of fakes inside at least one real ball            density   sum over fakes of #real balls it is in / (k |G|)
  coverage   the fraction of reals whose ball holds at least one fake       recall    the fraction of reals inside at least one fake ball"""
import numpy as np

from nn_ref import images                                                  # noqa: F401  (the data of the tests)


def _rows(x):
    x = np.asarray(x)
    return x.reshape(len(x), -1).astype(np.int64)


def d2(a, b):
    """int64 [Na,Nb], one row at a time: sum_d (a[p, d] - b[c, d])^2."""
    a, b = _rows(a), _rows(b)
    return np.stack([((b - p[None]) ** 2).sum(axis=1) for p in a])


def radii(x, k):
    """int64 [N]: for every image the k-th smallest distance to the images at the OTHER indices."""
    dist = d2(x, x)
    n = len(dist)
    assert 1 <= k <= n - 1
    return np.array([sorted(int(dist[i, j]) for j in range(n) if j != i)[k - 1] for i in range(n)], dtype=np.int64)


def block_candidates(x, k, tile):
    """int64 [N][ceil(N / tile)][k]: the k smallest distances of row i within every block of ``tile`` columns, j != i, ascending, padded
    with INT64_MAX (what pg_prd_kth_u8 leaves for the second launch)."""
    dist = d2(x, x)
    n = len(dist)
    blocks = (n + tile - 1) // tile
    out = np.full((n, blocks, k), np.iinfo(np.int64).max, dtype=np.int64)
    for i in range(n):
        for g in range(blocks):
            vals = sorted(int(dist[i, j]) for j in range(g * tile, min(n, (g + 1) * tile)) if j != i)[:k]
            out[i, g, :len(vals)] = vals
    return out


def ball_counts(a, b, rad_a=None, rad_b=None):
    """(a_cnt [Na], a_hit [Na], b_cnt [Nb], b_hit [Nb]) as lists of ints, None where the radius vector is None:
    a_cnt[p] = #{c : d2 <= rad_b[c]}, b_hit[c] = #{p : d2 <= rad_b[c]}, b_cnt[c] = #{p : d2 <= rad_a[p]}, a_hit[p] = #{c : d2 <= rad_a[p]}."""
    dist = d2(a, b)
    na, nb = dist.shape
    a_cnt = b_hit = b_cnt = a_hit = None
    if rad_b is not None:
        a_cnt = [sum(1 for c in range(nb) if dist[p, c] <= int(rad_b[c])) for p in range(na)]
        b_hit = [sum(1 for p in range(na) if dist[p, c] <= int(rad_b[c])) for c in range(nb)]
    if rad_a is not None:
        b_cnt = [sum(1 for p in range(na) if dist[p, c] <= int(rad_a[p])) for c in range(nb)]
        a_hit = [sum(1 for c in range(nb) if dist[p, c] <= int(rad_a[p])) for p in range(na)]
    return a_cnt, a_hit, b_cnt, b_hit


def prd(reals, fakes, k):
    """{'precision', 'recall', 'density', 'coverage'} of fakes against reals."""
    fake_cnt, _, real_cnt, real_hit = ball_counts(fakes, reals, radii(fakes, k), radii(reals, k))
    ng, nr = len(fake_cnt), len(real_hit)
    return {'precision': sum(1 for v in fake_cnt if v > 0) / float(ng), 'density': sum(fake_cnt) / float(k * ng),
            'coverage': sum(1 for v in real_hit if v > 0) / float(nr), 'recall': sum(1 for v in real_cnt if v > 0) / float(nr)}


def two_clusters(seed=0):
    """(reals, fakes) of the issue's construction at D = 192: 40 reals with bytes in [0, 64) and 24 with bytes in [192, 256), 64 fakes in
    the first cluster only.  No ball of either set reaches across: the largest distance inside a cluster is 63^2 * 192 and the smallest
    between the clusters 129^2 * 192."""
    rs = np.random.RandomState(seed)
    near = rs.randint(0, 64, size=(40, 3, 8, 8)).astype(np.uint8)
    far = rs.randint(192, 256, size=(24, 3, 8, 8)).astype(np.uint8)
    fakes = rs.randint(0, 64, size=(64, 3, 8, 8)).astype(np.uint8)
    return np.concatenate([near, far]), fakes
