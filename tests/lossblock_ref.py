"""fp64 references and derived per-element bounds for the WGAN-GP loss block (``pg_gp_mix``, ``pg_row_sumsq``, ``pg_gp_seed``,
``pg_d_loss``, ``pg_g_loss``) and the ``pg_linear1_*`` kernels (test infrastructure: tests/test_lossblock_gpu.py holds the kernels to
them, tests/test_lossblock_host.py ties them to float64 autograd of the reference's expressions).

Every reference takes host copies of the fp32 operands, rounds the scalar arguments to fp32 as the C ABI does, forms derived scalars in
fp32 where the kernel does (``1 - m[n]``, ``1 / N``) and evaluates everything else in fp64.  Every bound follows the kernel's operation
sequence in csrc/elementwise.hip: u = 2^-24 relative per add, multiply and fma, 2u per sqrtf and per division, propagated to first order;
a sum is charged (longest chain of additions a term passes through) x u x (sum of the terms' magnitudes).  A contracted fma rounds once
where two charges are made here.  The dropped products of charges are below (chain length x u) times the bound; the longest chain here
has 315 additions (2^-15.7), so every bound is widened by (1 + 2^-14).  Nothing is fitted to an observed error."""
import numpy as np

U = 2.0 ** -24
WIDEN = 1.0 + 2.0 ** -14


def f32(x):
    return float(np.float32(x))


def _d(x):
    return np.asarray(x, np.float64)


# ------------------------------------------------------------------------------------------------------------- launch geometry
def _grid(total, per_block, cap):
    return max(1, min((total + per_block - 1) // per_block, cap))


def row_sumsq_chain(E):
    """Longest chain of additions of ``pg_row_sumsq`` for E floats per row (include/pggan_hip.h and the launch in pg_row_sumsq: float4
    loads, 256 threads, at most 256 workgroups of 8 float4 per thread): the terms one thread accumulates (4 per float4, grid-stride
    loop), 6 shuffle levels, 4 waves, one atomic add per workgroup; + 1 for the rounding of the square itself."""
    e4 = E // 4
    blocks = _grid(e4, 256 * 8, 256)
    per_thread = -(-e4 // (blocks * 256))
    return 4 * per_thread + 6 + 4 + blocks + 1


def gp_blocks(E):
    """Workgroups per row of ``pg_gp_mix`` / ``pg_gp_seed``: one float4 per thread, 256 threads, capped at 1024 (grid-stride beyond)."""
    return _grid(E // 4, 256, 1024)


# ------------------------------------------------------------------------------------------------------------------ loss block
def row_sumsq(g, ss0=None):
    """ss[n] (+ what ``ss`` held: the kernel accumulates) and its bound k u (|ss0| + sum x^2)."""
    g = _d(g).reshape(g.shape[0], -1)
    ss0 = np.zeros(g.shape[0]) if ss0 is None else _d(ss0)
    s = (g * g).sum(1)
    return ss0 + s, row_sumsq_chain(g.shape[1]) * U * (np.abs(ss0) + s) * WIDEN


def gp_mix(real, fake, m):
    """mixed = real * mr + fake * m[n] with mr = fl(1 - m[n]); bound u |real mr| + u |fake m| + u |mixed|."""
    N = real.shape[0]
    r, f = _d(real).reshape(N, -1), _d(fake).reshape(N, -1)
    mf = _d(m).reshape(N, 1)
    mr = (np.float32(1) - np.asarray(m, np.float32).reshape(N, 1)).astype(np.float64)
    a, b = r * mr, f * mf
    return a + b, U * (np.abs(a) + np.abs(b) + np.abs(a + b)) * WIDEN


def gp_seed(g, ss, lam, target, inv_n):
    """gp[n] = lam (sqrt(ss[n]) - target)^2 / target^2 and the seed u[n,e] = inv_n d gp[n] / d g[n,e]
    = inv_n 2 lam (norm - target) / (target^2 norm) g[n,e], DEFINED AS 0 WHERE norm == 0 (the subgradient autograd takes for
    ``norm``; the kernel's ``norm > 0`` branch).  ``ss`` is an operand (fp32, exact).

    norm = sqrtf(ss): e_norm = 2u norm.  d = norm - target: e_d = e_norm + u |d|.
    gp = ((d d) lam) / (target target): the square carries 2 |d| e_d + e_d^2, then d d, x lam, target^2 (u each) and the division (2u).
    coef = (((inv_n 2) lam) d) / ((target target) norm): x lam, x d, target^2, x norm (u each), the division (2u), plus e_d through the
    numerator and e_norm through the denominator.  u = g coef: one more u."""
    N = g.shape[0]
    lam, target, inv_n = f32(lam), f32(target), f32(inv_n)
    g, ss = _d(g).reshape(N, -1), _d(ss)
    norm = np.sqrt(ss)
    d = norm - target
    e_norm = 2 * U * norm
    e_d = e_norm + U * np.abs(d)
    gp = d * d * lam / (target * target)
    e_gp = lam / (target * target) * (2 * np.abs(d) * e_d + e_d * e_d) + 5 * U * gp
    with np.errstate(divide='ignore', invalid='ignore'):
        coef = np.where(norm > 0, inv_n * 2 * lam * d / (target * target * norm), 0.0)
        e_coef = np.where(norm > 0, inv_n * 2 * lam * e_d / (target * target * norm) + np.abs(coef) * (6 * U + e_norm / norm), 0.0)
    u = g * coef[:, None]
    e_u = np.abs(g) * e_coef[:, None] + U * np.abs(u)
    return gp, e_gp * WIDEN, u, e_u * WIDEN


def d_loss(s, gp, N, eps):
    """scores s = [real(N) | fake(N) | mixed(N)] -> dict name -> (value, bound) for d_cost, d_real_loss, d_fake_loss, gscore.

    invn = fl(1 / N) (u).  rl = -sr + (sr sr) eps: u for the square, u for x eps, u for the sum.  d_fake_loss = sf (a copy).
    d_cost = invn sum_n ((sf + rl) + gp): each term carries e_rl and two additions; one lane adds ceil(N / 64) terms, then 6 shuffle
    levels; then x invn (u) with invn's own u.  gscore[n] = (-1 + (2 eps) sr) invn: u for x sr, u for the sum, u for x invn, u of invn;
    gscore[N + n] = invn (u); gscore[2N + n] = 0."""
    eps = f32(eps)
    s, gp = _d(s), _d(gp)
    sr, sf = s[:N], s[N:2 * N]
    sq = sr * sr * eps
    rl = -sr + sq
    e_rl = 2 * U * np.abs(sq) + U * np.abs(rl)
    t = sf + rl + gp
    e_t = e_rl + U * np.abs(sf + rl) + U * np.abs(t)
    chain = -(-N // 64) + 6
    d_cost = t.sum() / N
    e_cost = (e_t.sum() + chain * U * np.abs(t).sum()) / N + 2 * U * abs(d_cost)
    lin = -1 + 2 * eps * sr
    gs = np.concatenate([lin / N, np.full(N, 1.0 / N), np.zeros(N)])
    e_gs = np.concatenate([(U * np.abs(2 * eps * sr) + U * np.abs(lin)) / N + 2 * U * np.abs(lin) / N, np.full(N, U / N), np.zeros(N)])
    return dict(d_cost=(d_cost, e_cost * WIDEN), d_real_loss=(rl, e_rl * WIDEN), d_fake_loss=(sf.copy(), np.zeros(N)),
                gscore=(gs, e_gs * WIDEN))


def g_loss(s):
    """g_cost = mean(-s): one lane subtracts ceil(N / 64) scores, 6 shuffle levels, x fl(1 / N); gscore[n] = -fl(1 / N)."""
    s = _d(s)
    N = s.shape[0]
    g_cost = -s.sum() / N
    e = (-(-N // 64) + 6) * U * np.abs(s).sum() / N + 2 * U * abs(g_cost)
    return g_cost, e * WIDEN, np.full(N, -1.0 / N), np.full(N, U / N) * WIDEN


# ------------------------------------------------------------------------------------------------------------------ Linear(C, 1)
def linear1_fwd(h, w, b):
    """s[n] = sum_c h[n,c] w[c] + b: one lane chains ceil(C / 64) fmas, 6 shuffle levels, one addition of the bias."""
    N = h.shape[0]
    h, w = _d(h).reshape(N, -1), _d(w).reshape(-1)
    b = 0.0 if b is None else float(_d(b).reshape(-1)[0])
    C = w.shape[0]
    s = h @ w + b
    return s, (-(-C // 64) + 6 + 1) * U * (np.abs(h) @ np.abs(w) + abs(b)) * WIDEN


def linear1_bwd_data(gs, w, mask, mask_slope):
    """gh[n,c] = gs[n] w[c] (mask ? (mask[n,c] > 0 ? 1 : slope) : 1): u per product."""
    gs, w = _d(gs).reshape(-1, 1), _d(w).reshape(1, -1)
    v = gs * w
    if mask is not None:
        v = v * np.where(_d(mask).reshape(v.shape) > 0, 1.0, f32(mask_slope))
    return v, 2 * U * np.abs(v) * WIDEN


def linear1_wgrad(gs, h, dw0, db0):
    """dw[c] += sum_n gs[n] h[n,c] (a chain of N fmas, one addition into dw); db += sum_n gs[n] (N additions, one into db)."""
    N = gs.shape[0]
    gs, h = _d(gs).reshape(N), _d(h).reshape(N, -1)
    dw0 = _d(dw0).reshape(-1)
    dw = dw0 + gs @ h
    e_dw = (N + 1) * U * (np.abs(dw0) + np.abs(gs) @ np.abs(h)) * WIDEN
    if db0 is None:
        return dw, e_dw, None, None
    db0 = float(_d(db0).reshape(-1)[0])
    return dw, e_dw, db0 + gs.sum(), (N + 1) * U * (abs(db0) + np.abs(gs).sum()) * WIDEN
