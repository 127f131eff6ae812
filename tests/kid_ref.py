"""TEST INFRASTRUCTURE: the tile sums of the cubic polynomial kernel and the unbiased MMD^2 estimator, restated for the CPU
(include/pggan_hip_kid.h): an int64 evaluation for data that rounds nowhere, an evaluation with exactly rounded
sums (math.fsum over the exact products) with the error bound of ANY fp64 evaluation order beside it, and the estimator as a plain
double loop over all pairs."""
import math

import numpy as np

TILE = 64
U = 2.0 ** -53                                                          # the unit roundoff of fp64
SLACK = 1.01                                                            # covers every second-order term below: (1 + 512 U)^k - 1 << 0.01


def tile_reduce(k, reduce=None):
    """[M,N] values per pair -> [ceil(M / 64), ceil(N / 64)] per tile; ``reduce`` None: numpy's sum (exact for integers), else a
    function of a flat list (math.fsum)."""
    M, N = k.shape
    A, B = (M + TILE - 1) // TILE, (N + TILE - 1) // TILE
    if reduce is None:
        padded = np.zeros((A * TILE, B * TILE), dtype=k.dtype)
        padded[:M, :N] = k
        return padded.reshape(A, TILE, B, TILE).sum(axis=(1, 3))
    return np.array([[reduce(k[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE].reshape(-1).tolist()) for b in range(B)] for a in range(A)])


def tilesums_int(x, y=None, gamma=1, coef0=1, skip_diagonal=False):
    """Integer features, integer gamma and coef0: the tile sums in int64, exact."""
    xi = np.asarray(x).astype(np.int64)
    yi = xi if y is None else np.asarray(y).astype(np.int64)
    assert (xi == np.asarray(x)).all() and (yi == np.asarray(x if y is None else y)).all()
    k = (int(gamma) * xi.dot(yi.T) + int(coef0)) ** 3
    if skip_diagonal:
        assert y is None
        np.fill_diagonal(k, 0)
    return tile_reduce(k)


def pairs_exact(x, y=None, gamma=None, coef0=1.0):
    """(k [M,N], bound [M,N]) for float32 features: k = (t t) t, t = gamma g + coef0 in fp64 from g = the exactly rounded sum of the
    exact products (math.fsum; a product of two float32 values is exact in fp64), and the bound on |k_device - k| + (the share of a
    pair in the summation error of its tile) for a device that evaluates in fp64 in ANY order.  With G = sum_f |x_f y_f|,
    T = |gamma| G + |coef0| >= |t| and c additions in g (c = F on the device, c = 1 rounding here):
        |g^ - g| <= c U G                                               (c additions, each within U of its exact value)
        |t^ - t| <= e_t(c) = c U |gamma| G + 2 U T                      (one multiplication and one addition, each within U)
        |k^ - k| <= e_k(c) = 3 T^2 e_t(c) + 2 U T^3                     (the derivative of t^3, and two multiplications)
    and a sum of at most 4096 such values in any order is within 4096 U sum |k^| of their exact sum, the exactly rounded sum of this
    file within 1 U: bound = SLACK (e_k(F) + e_k(1) + 4097 U T^3), SLACK for the second-order terms."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    self_form = y is None
    y64 = x64 if self_form else np.asarray(y, dtype=np.float32).astype(np.float64)
    (M, F), N = x64.shape, y64.shape[0]
    gamma = 1.0 / F if gamma is None else float(gamma)
    g, G = np.empty((M, N)), np.empty((M, N))
    for i in range(M):
        j0 = i if self_form else 0
        p = x64[i] * y64[j0:]                                           # exact
        g[i, j0:] = [math.fsum(row) for row in p.tolist()]
        G[i, j0:] = np.abs(p).sum(axis=1)
        if self_form:
            g[i:, i], G[i:, i] = g[i, i:], G[i, i:]
    G = G * (1 + F * U)                                                 # (the sum of magnitudes is itself rounded: an upper bound)
    t = gamma * g + coef0
    k = (t * t) * t
    T = abs(gamma) * G + abs(coef0)
    e_t = lambda c: c * U * abs(gamma) * G + 2 * U * T
    e_k = lambda c: 3 * T * T * e_t(c) + 2 * U * T ** 3
    return k, SLACK * (e_k(F) + e_k(1) + 4097 * U * T ** 3)


def tilesums_exact(x, y=None, gamma=None, coef0=1.0, skip_diagonal=False):
    """(sums [A,B], bound [A,B]): the tile sums with exactly rounded sums, and what any fp64 evaluation may differ from them by."""
    k, bound = pairs_exact(x, y, gamma, coef0)
    if skip_diagonal:
        assert y is None
        np.fill_diagonal(k, 0.0)
        np.fill_diagonal(bound, 0.0)
    return tile_reduce(k, math.fsum), tile_reduce(bound) * SLACK


def kid_loops(kxx, kyy, kxy):
    """The unbiased MMD^2 estimator from the kernel values of all pairs as plain double loops, and the sum of the magnitudes of its
    terms (what a rounding error of the evaluation scales with)."""
    m, n = kxx.shape[0], kyy.shape[0]
    sxx = math.fsum(kxx[i, j] for i in range(m) for j in range(m) if i != j)
    syy = math.fsum(kyy[i, j] for i in range(n) for j in range(n) if i != j)
    sxy = math.fsum(kxy[i, j] for i in range(m) for j in range(n))
    mag = (np.abs(kxx).sum() / (m * (m - 1.0)) + np.abs(kyy).sum() / (n * (n - 1.0)) + 2.0 * np.abs(kxy).sum() / (float(m) * n))
    return sxx / (m * (m - 1.0)) + syy / (n * (n - 1.0)) - 2.0 * sxy / (float(m) * n), float(mag)


def kid_bound(bxx, byy, bxy, sxx, syy, sxy, m, n):
    """What ``kid_statistic`` over tile sums within ``b*`` of ``s*`` may differ by from ``kid_statistic`` over ``s*``: the tile bounds
    through the three quotients, and the host's own arithmetic -- a numpy sum over the tiles, a division, two additions: fewer than
    (number of tiles + 4) roundings on the path of any term."""
    through = bxx.sum() / (m * (m - 1.0)) + byy.sum() / (n * (n - 1.0)) + 2.0 * bxy.sum() / (float(m) * n)
    mag = np.abs(sxx).sum() / (m * (m - 1.0)) + np.abs(syy).sum() / (n * (n - 1.0)) + 2.0 * np.abs(sxy).sum() / (float(m) * n)
    return float(SLACK * (through + 2 * (max(sxx.size, syy.size, sxy.size) + 4) * U * mag))
