"""fp64 references and derived per-element bounds for the normalisation and pooling kernels of csrc/elementwise.hip: PixelNorm
(``pg_pixelnorm_fwd`` / ``_lrelu_bwd`` / ``_tangent`` / ``_lrelu_bwd_inj``), minibatch stddev (``pg_mbstd_fwd`` / ``_tangent`` / ``_bwd`` and
the six exact-global entry points) and ``pg_avgpool2_fwd`` / ``_bwd``, ``pg_upsample2_bwd``, ``pg_axpby_mask`` (test infrastructure:
tests/test_normalisation_gpu.py holds the kernels to them, tests/test_normalisation_host.py ties them to float64 autograd).

Every reference takes host copies of the fp32 operands, rounds the scalar arguments to fp32 as the C ABI does and evaluates the contract
sentence of include/pggan_hip.h in fp64.  A tensor that a kernel reads from an earlier launch (``y``, ``r``, ``stats``, ``tstats``,
``gsums``) is an operand: it goes in as the device produced it, and has its own assertion against fp64 where it is produced.

Every bound follows the kernel's operation sequence: u = 2^-24 relative per add, multiply and fma, 2u per sqrtf, rsqrtf and division,
propagated to first order; a sum is charged (longest chain of additions a term passes through) x u x (sum of the terms' magnitudes), the
chain counted from the launch geometry (``pn_chain``, ``mb_slices``, ``rows_chain``).  A contracted fma rounds once where two charges are
made here.  The dropped products of charges are below (chain x u) times the bound; the longest chain here is 4 x 2 + 10 + 96 + 2 = 116
(the tangent's dot product over three ranks, 2^-17.1), so every bound is widened by (1 + 2^-14).  The one place where an error enters
SQUARED at a size that matters -- the slice means inside the minibatch variance, at |mean| >> sigma -- carries its quadratic term
explicitly (``_merge``).  Masks follow the header: ``m > 0 ? 1 : slope``, so 0.0 and -0.0 take the slope.  Nothing is fitted to an
observed error."""
import numpy as np

U = 2.0 ** -24
WIDEN = 1.0 + 2.0 ** -14
MB_PARTS = 32                                # workgroups (= slices) per group of the minibatch-stddev launches
MB_EPS = float(np.float32(1.0e-8))           # the constant inside sqrt(var + 1e-8), an fp32 literal in the kernel
GRID_CAP = 4096                              # grid_for: at most 4096 workgroups of 256 threads, grid-stride beyond


def f32(x):
    return float(np.float32(x))


def _d(x):
    return np.asarray(x, np.float64)


def _lrelu_factor(m, slope):
    """The header's mask: (m > 0 ? 1 : slope); 0.0 and -0.0 take the slope."""
    return np.where(_d(m) > 0, 1.0, f32(slope))


def _masked(v, e, m, slope):
    """v * factor: exact where the factor is 1, one rounding (u) where it is the slope."""
    k = _lrelu_factor(m, slope)
    out = v * k
    return out, np.where(k == 1.0, e, np.abs(k) * e + U * np.abs(out))


# ------------------------------------------------------------------------------------------------------------- launch geometry
def pick_lpp(C):
    """Lanes per pixel of the general PixelNorm kernels: the smallest power of two >= C / 4, at most 64."""
    c4, l = C // 4, 1
    while l < c4 and l < 64:
        l *= 2
    return l


def pn_narrow(C):
    """``pg_pixelnorm_lrelu_bwd`` / ``_inj`` take the one-thread-per-pixel kernel at C = 8 and 16."""
    return C in (8, 16)


def pn_chain(C, narrow=False):
    """Longest chain of additions of one per-pixel dot product: 4 per float4 a lane visits (three inside the float4, one into the
    accumulator), ceil(C4 / LPP) float4 per lane, log2(LPP) shuffle levels of group_sum<LPP>; the narrow kernel adds its C4 float4 in
    one thread.  + 1 for the rounding of each product is added where the chain is used."""
    c4 = C // 4
    if narrow:
        return 4 * c4
    lpp = pick_lpp(C)
    return 4 * (-(-c4 // lpp)) + int(np.log2(lpp))


def pn_wraps(P, C, narrow=False):
    """True where the launch's grid-stride loop takes a second turn (the cap of the narrow kernel is 2^20 workgroups)."""
    return P > (1 << 28) if narrow else P * pick_lpp(C) > GRID_CAP * 256


def mb_slices(M4):
    """(begin, end) in float4 of the MB_PARTS slices of one group (mb_slice: ceil(M4 / 32) each, a ragged last one, empty ones behind)."""
    per = -(-M4 // MB_PARTS)
    out = []
    for i in range(MB_PARTS):
        b = i * per
        e = min(b + per, M4)
        out.append((min(b, M4), e))
    return out


def _block_chain(n4, per_float4):
    """Chain of a 256-thread block_sum over n4 float4: per_float4 additions per float4 a thread visits, 6 shuffle levels, 4 waves."""
    return per_float4 * (-(-n4 // 256)) + 6 + 4


def rows_chain(rows):
    """Chain of the sum over the rows of channel C (mbstd_bwd_kernel, mbstd_gsum_kernel): ceil(rows / 256) per thread, 6 levels, 4 waves."""
    return -(-rows // 256) + 6 + 4


# ------------------------------------------------------------------------------------------------------------------- PixelNorm
def pixelnorm_fwd(x, eps=1e-8):
    """r = rsqrt(mean_c x^2 + eps), y = x r -> (y, e_y, r, e_r).

    s = sum x^2: (chain + 1) u s.  m = s / C: 2u.  v = m + eps: u.  r = rsqrtf(v): 2u r + r e_v / (2 v).  y = x r: |x| e_r + u |y|."""
    x = _d(x)
    C = x.shape[-1]
    eps = f32(eps)
    s = (x * x).sum(-1)
    e_s = (pn_chain(C) + 1) * U * s
    m = s / C
    e_m = e_s / C + 2 * U * m
    v = m + eps
    e_v = e_m + U * v
    r = 1.0 / np.sqrt(v)
    e_r = r * (2 * U + e_v / (2 * v))
    y = x * r[..., None]
    e_y = np.abs(x) * e_r[..., None] + U * np.abs(y)
    return y, e_y * WIDEN, r, e_r * WIDEN


def pixelnorm_lrelu_bwd(gy, y, r, slope, inj=None, mutate=None):
    """gz = (r (gy - y mean_c(gy y)) + inj) (y > 0 ? 1 : slope) from the saved y, r; r None: gz = gy (y > 0 ? 1 : slope).

    s = sum gy y: (chain + 1) u sum|gy y|.  mean = s / C: 2u.  o = r (gy - y mean): |y| e_mean + u |y mean| for the product, u for the
    difference, u for x r; + inj: u; the slope: u.  ``mutate``: 'proj' scales the projection term by 1.05, 'inj' the injection."""
    gy, y = _d(gy), _d(y)
    C = y.shape[-1]
    if r is None:
        gz, e = _masked(gy, np.zeros_like(gy), y, slope)
        return gz, e * WIDEN
    r = _d(r).reshape(y.shape[:-1])[..., None]
    k = pn_chain(C, pn_narrow(C)) + 1
    s = (gy * y).sum(-1, keepdims=True)
    e_s = k * U * np.abs(gy * y).sum(-1, keepdims=True)
    mean = s / C
    e_mean = e_s / C + 2 * U * np.abs(mean)
    p = y * mean * (1.05 if mutate == 'proj' else 1.0)
    o = r * (gy - p)
    e_o = r * (np.abs(y) * e_mean + U * np.abs(p) + U * np.abs(gy - p)) + U * np.abs(o)
    if inj is not None:
        o = o + _d(inj) * (1.05 if mutate == 'inj' else 1.0)
        e_o = e_o + U * np.abs(o)
    gz, e = _masked(o, e_o, y, slope)
    return gz, e * WIDEN


def pixelnorm_tangent(t, y, r, a, mutate=None):
    """ty = P t and inj = -(r^2 S / C) y - (r / C) P[(a.y) t + (t.y) a], P = r (I - y y^T / C), S = t.a - (t.y)(a.y) / C
    -> (ty, e_ty, inj, e_inj), following pixelnorm_tangent_kernel:

    the three dot products: (chain + 1) u sum|.|;  invC = 1 / C: 2u
    ty = r (t - (y ty_) invC): the product 4u |p| + |y| e_ty / C, u for the difference, u for x r
    S = ta - (ty_ ay_) invC;  k_y = -(((r r) S) invC): 5u + r^2 e_S / C;  yd = (2 ay_) ty_;  kp = -(r invC) r: 4u
    inj = k_y y + kp ((ay_ t + ty_ a) - (y yd) invC): u per product and per sum, 4u for the invC product.
    ``mutate``: 'k_y' / 'kp' scale that coefficient by 1.05."""
    t, y, a = _d(t), _d(y), _d(a)
    C = y.shape[-1]
    r = _d(r).reshape(y.shape[:-1])[..., None]
    k = pn_chain(C) + 1
    dot = lambda p, q: ((p * q).sum(-1, keepdims=True), k * U * np.abs(p * q).sum(-1, keepdims=True))
    (ty_, e_ty), (ay_, e_ay), (ta_, e_ta) = dot(t, y), dot(a, y), dot(t, a)
    p = y * ty_ / C
    e_p = np.abs(y) * e_ty / C + 4 * U * np.abs(p)
    o = r * (t - p)
    e_o = r * (e_p + U * np.abs(t - p)) + U * np.abs(o)
    q = ty_ * ay_ / C
    e_q = (np.abs(ay_) * e_ty + np.abs(ty_) * e_ay) / C + 4 * U * np.abs(q)
    S = ta_ - q
    e_S = e_ta + e_q + U * np.abs(S)
    k_y = -(r * r * S / C) * (1.05 if mutate == 'k_y' else 1.0)
    e_ky = r * r * e_S / C + 5 * U * np.abs(k_y)
    yd = 2 * ay_ * ty_
    e_yd = 2 * (np.abs(ay_) * e_ty + np.abs(ty_) * e_ay) + U * np.abs(yd)
    kp = -(r / C) * r * (1.05 if mutate == 'kp' else 1.0)
    e_kp = 4 * U * np.abs(kp)
    A, B, Cc = ay_ * t, ty_ * a, y * yd / C
    e_A = np.abs(t) * e_ay + U * np.abs(A)
    e_B = np.abs(a) * e_ty + U * np.abs(B)
    e_C = np.abs(y) * e_yd / C + 4 * U * np.abs(Cc)
    inner = (A + B) - Cc
    e_in = e_A + e_B + U * np.abs(A + B) + e_C + U * np.abs(inner)
    j = k_y * y + kp * inner
    e_j = np.abs(y) * e_ky + U * np.abs(k_y * y) + np.abs(inner) * e_kp + np.abs(kp) * e_in + U * np.abs(kp * inner) + U * np.abs(j)
    return o, e_o * WIDEN, j, e_j * WIDEN


# ------------------------------------------------------------------------------------------------------------ minibatch stddev
def _slice_partials(xg):
    """Partials {count, mean, M2} of the 32 slices of one shard of one group, as mbstd_stats_kernel forms them, with their bounds:
    (c, m, e_m, q, e_q) per slice.

    mean = block_sum(sum x) / c: (3 per float4 + 6 + 4) additions, 2u for the division -> e_m = (chain + 2) u mean|x|.
    q = block_sum(sum (x - m~)^2) around the COMPUTED mean m~ = m + d, |d| <= e_m: sum (x - m~)^2 = M2 + c d^2 exactly; each term carries
    2u (the difference, squared) + u (the square), then the same chain."""
    xg = xg.reshape(-1)
    out = []
    for b, e in mb_slices(xg.size // 4):
        seg = xg[4 * b:4 * e]
        c = seg.size
        if c == 0:
            out.append((0, 0.0, 0.0, 0.0, 0.0))
            continue
        chain = _block_chain(e - b, 3)
        m = seg.mean()
        e_m = (chain + 2) * U * np.abs(seg).mean()
        q = ((seg - m) ** 2).sum()
        e_q = c * e_m ** 2 + (chain + 3) * U * (q + c * e_m ** 2)
        out.append((c, m, e_m, q, e_q))
    return out


def _merge(partials, M):
    """Chan's merge of the partials in the kernel's order (mb_merge: rank-major, slice by slice, empty slices skipped), in fp64, with
    the bound carried along -> (mu, e_mu, sigma, e_sigma).  Per step, with d = m - mean, f = c / tot, w = cnt c / tot:

    mean += d f:       e_mean' = (1 - f) e_mean + f e_m + (u |d| + 3u |d|) f + u |mean'|           (the difference, c / tot, the product; the sum)
    m2 += q + d d w:   e_d = e_m + e_mean + u |d| enters as w (2 |d| e_d + e_d^2) -- the square is kept: at |mean| >> sigma e_d is
                       of the size of d itself --, 5u for (d d)(cnt c / tot), u for q + t, u for the sum into m2.
    sigma = sqrtf(m2 / M + 1e-8): 2u for the division, u for the sum, 2u for the root; e_var passes through the root as
    e_var / (sqrt(var) + sqrt(var - e_var))."""
    cnt = mean = m2 = e_mean = e_m2 = 0.0
    for c, m, e_m, q, e_q in partials:
        if c == 0:
            continue
        tot = cnt + c
        d = m - mean
        f = c / tot
        e_d = e_m + e_mean + U * abs(d)
        new_mean = mean + d * f
        w = cnt * c / tot
        t = d * d * w
        T = w * (abs(d) + e_d) ** 2
        e_t = (T - t) + 5 * U * T
        new_m2 = m2 + q + t
        e_m2 = e_m2 + e_q + e_t + U * (q + e_q + T) + U * (new_m2 + e_m2 + e_q + e_t)
        e_mean = (1 - f) * e_mean + f * e_m + 4 * U * abs(d) * f + U * (abs(new_mean) + e_mean + e_m)
        cnt, mean, m2 = tot, new_mean, new_m2
    assert cnt == M
    var = m2 / M + MB_EPS
    e_var = e_m2 / M + 2 * U * m2 / M + U * var
    sigma = np.sqrt(var)
    e_sigma = e_var / (sigma + np.sqrt(max(var - e_var, 0.0))) + 2 * U * sigma
    return mean, e_mean * WIDEN, sigma, e_sigma * WIDEN


def mbstd_stats(shards, G):
    """mu and sigma = sqrt(mean((x - mu)^2) + 1e-8) per group over all ``shards`` (a list of [G * n_r, H, W, C] arrays, one per rank; a
    single-process call is a list of one) -> (mu[G], e_mu[G], sigma[G], e_sigma[G])."""
    shards = [_d(s).reshape(G, -1) for s in shards]
    M = sum(s.shape[1] for s in shards)
    rows = [_merge([p for s in shards for p in _slice_partials(s[g])], M) for g in range(G)]
    return tuple(np.array(col) for col in zip(*rows))


def mbstd_fwd(x, G, cp, shards=None):
    """y[..., :C] = x, y[..., C] = sigma_g, channels behind it 0 -> (y, e_y, mu, e_mu, sigma, e_sigma).  ``shards``: the arrays of all
    ranks in exact-global mode (x is then this rank's)."""
    x = _d(x)
    NB, C = x.shape[0], x.shape[-1]
    mu, e_mu, sigma, e_sigma = mbstd_stats([x] if shards is None else shards, G)
    y = np.zeros(x.shape[:-1] + (cp,))
    e_y = np.zeros_like(y)
    y[..., :C] = x
    y[..., C] = np.repeat(sigma, NB // G).reshape((NB,) + (1,) * (x.ndim - 2))
    e_y[..., C] = np.repeat(e_sigma, NB // G).reshape((NB,) + (1,) * (x.ndim - 2))
    return y, e_y, mu, e_mu, sigma, e_sigma


def mbstd_tangent(tx, stats, G, cp, shards):
    """ty[..., :C] = tx, ty[..., C] = <x - mu, tx> / (M sigma); tstats = {mean(tx), <x - mu, tx>} -> (ty, e_ty, tmean, e_tmean, dot, e_dot).
    ``shards``: [(x_r, tx_r)] of every rank (one pair for a single-process call); ``stats`` [G, >= 2]: mu, sigma as the device holds them.

    Slice partials: sum tx has 3 additions per float4 + 6 + 4, the dot product 4 + 6 + 4 with 2u per term ((x - mu), the product); the
    write kernel adds the 32 x nranks partials one after the other.  tmean = ts / M: 2u.  ty_C = dot / (M sigma): u, 2u."""
    tx, stats = _d(tx), _d(stats)
    NB, C = tx.shape[0], tx.shape[-1]
    xs = [_d(s[0]).reshape(G, -1) for s in shards]
    ts = [_d(s[1]).reshape(G, -1) for s in shards]
    M = sum(s.shape[1] for s in xs)
    K = MB_PARTS * len(shards)
    it = max(-(-(e - b) // 256) for s in xs for b, e in mb_slices(s.shape[1] // 4))
    mu, sigma = stats[:, 0], stats[:, 1]
    tsum = sum(t.sum(1) for t in ts)
    e_tsum = (3 * it + 10 + K) * U * sum(np.abs(t).sum(1) for t in ts)
    tmean = tsum / M
    e_tmean = e_tsum / M + 2 * U * np.abs(tmean)
    dot = sum(((x - mu[:, None]) * t).sum(1) for x, t in zip(xs, ts))
    e_dot = (4 * it + 10 + K + 2) * U * sum(np.abs((x - mu[:, None]) * t).sum(1) for x, t in zip(xs, ts))
    val = dot / (M * sigma)
    e_val = e_dot / (M * sigma) + 3 * U * np.abs(val)
    ty = np.zeros(tx.shape[:-1] + (cp,))
    e_ty = np.zeros_like(ty)
    ty[..., :C] = tx
    ty[..., C] = np.repeat(val, NB // G).reshape((NB,) + (1,) * (tx.ndim - 2))
    e_ty[..., C] = np.repeat(e_val * WIDEN, NB // G).reshape((NB,) + (1,) * (tx.ndim - 2))
    return ty, e_ty, tmean, e_tmean * WIDEN, dot, e_dot * WIDEN


def mbstd_gsum(g, G, C):
    """sum over the rows of g[..., C] per group ([G * n, H, W, CP]; None -> zeros) -> (sum[G], bound[G])."""
    if g is None:
        return np.zeros(G), np.zeros(G)
    col = _d(g)[..., C].reshape(G, -1)
    return col.sum(1), rows_chain(col.shape[1]) * U * np.abs(col).sum(1) * WIDEN


def mbstd_bwd(gy, x, stats, G, apply_mask, mask_slope=0.2, tx=None, tstats=None, gy_first=None, gsums=None, nranks=1, mutate=None):
    """gx = (gy[..., :C] + Gs (x - mu) / (M sigma) + hvp) (x > 0 ? 1 : slope),
    hvp = Gs1 / (M sigma) ((tx - mean tx) - (x - mu) <x - mu, tx> / (M sigma^2)) -> (gx, bound).

    ``stats`` / ``tstats`` [G, >= 2] as the device holds them.  ``gsums`` None: Gs / Gs1 are the sums over this call's rows, charged
    their chain; [G, 2]: operands (exact-global mode, M = nranks x this shard).
    invMs = 1 / ((M nranks) sigma): 3u.  k1 = Gs invMs, k2 = Gs1 invMs: + u.  k3 = (k2 dot) / (((M nranks) sigma) sigma): 5u.
    kx = k1 - k3: u.  gx = gy_c + kx (x - mu) + k2 (tx - tmean): 2u per product (difference, product), u per sum; the slope: u.
    ``mutate``: 'std' scales k1, 'hvp_t' the (tx - mean tx) piece, 'hvp_x' the (x - mu) piece of the hvp by 1.05."""
    x = _d(x)
    C = x.shape[-1]
    xg = x.reshape(G, -1, C)
    rows = xg.shape[1]
    M = float(rows * C * nranks)
    stats = _d(stats)
    mu, sigma = stats[:, 0].reshape(G, 1, 1), stats[:, 1].reshape(G, 1, 1)
    gyg = None if gy is None else _d(gy).reshape(G, rows, -1)
    if gsums is None:
        Gs, e_Gs = mbstd_gsum(gy, G, C)
        Gs1, e_Gs1 = mbstd_gsum(gy_first if tx is not None else None, G, C)
    else:
        gsums = _d(gsums)
        Gs, e_Gs = (gsums[:, 0] if gy is not None else np.zeros(G)), np.zeros(G)
        Gs1, e_Gs1 = (gsums[:, 1] if tx is not None else np.zeros(G)), np.zeros(G)
    Gs, e_Gs, Gs1, e_Gs1 = (v.reshape(G, 1, 1) for v in (Gs, e_Gs, Gs1, e_Gs1))
    inv = 1.0 / (M * sigma)
    k1 = Gs * inv * (1.05 if mutate == 'std' else 1.0)
    e_k1 = e_Gs * inv + 4 * U * np.abs(k1)
    k2 = Gs1 * inv
    e_k2 = e_Gs1 * inv + 4 * U * np.abs(k2)
    k3, e_k3 = np.zeros_like(k2), np.zeros_like(k2)
    if tx is not None:
        ts = _d(tstats)
        tmean, dot = ts[:, 0].reshape(G, 1, 1), ts[:, 1].reshape(G, 1, 1)
        k3 = k2 * dot / (M * sigma * sigma) * (1.05 if mutate == 'hvp_x' else 1.0)
        e_k3 = e_k2 * np.abs(dot / (M * sigma * sigma)) + 5 * U * np.abs(k3)
    kx = k1 - k3
    e_kx = e_k1 + e_k3 + U * np.abs(kx)
    v = np.zeros_like(xg) if gyg is None else gyg[..., :C].copy()
    a = kx * (xg - mu)
    v = v + a
    e = np.abs(xg - mu) * e_kx + 2 * U * np.abs(a) + U * np.abs(v)
    if tx is not None:
        dt = _d(tx).reshape(G, rows, C) - tmean
        b = k2 * dt * (1.05 if mutate == 'hvp_t' else 1.0)
        v = v + b
        e = e + np.abs(dt) * e_k2 + 2 * U * np.abs(b) + U * np.abs(v)
    if apply_mask:
        v, e = _masked(v, e, xg, mask_slope)
    return v.reshape(x.shape), (e * WIDEN).reshape(x.shape)


# ------------------------------------------------------------------------------------------------- pool / upsample / axpby
def _quad(x):
    """The four fine elements under every coarse one of an NHWC tensor, in the kernels' order p0 p1 / p2 p3."""
    x = _d(x)
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def avgpool2_fwd(x, other=None, a=1.0, b=0.0, mutate=None):
    """y = a avgpool2(x) + b other: v = ((p0 + p1) + (p2 + p3)) 0.25 -- u per sum, the quarter exact --, then fma(v, a, b other)
    (u for the product b other, u for the fma), or v a where other is absent and a != 1 (u).  ``mutate``: 'quarter' / 'b' x 1.05."""
    p0, p1, p2, p3 = _quad(x)
    a, b = f32(a), f32(b)
    s = (p0 + p1) + (p2 + p3)
    e_s = U * (np.abs(p0 + p1) + np.abs(p2 + p3) + np.abs(s))
    quarter = 0.25 * (1.05 if mutate == 'quarter' else 1.0)
    v, e_v = s * quarter, e_s * 0.25
    if other is not None:
        bq = b * (1.05 if mutate == 'b' else 1.0) * _d(other)
        y = v * a + bq
        return y, (abs(a) * e_v + U * np.abs(bq) + U * np.abs(y)) * WIDEN
    if a != 1.0:
        return v * a, (abs(a) * e_v + U * np.abs(v * a)) * WIDEN
    return v, e_v * WIDEN


def avgpool2_bwd(gy, mask=None, mul=1.0, mask_slope=0.2, mutate=None):
    """gx[n, h, w, c] = (mul 0.25) gy[n, h / 2, w / 2, c] (mask > 0 ? 1 : slope): k = mul 0.25 is exact, u for the product, u for the slope."""
    g = np.repeat(np.repeat(_d(gy), 2, axis=1), 2, axis=2)
    k = f32(mul) * 0.25 * (1.05 if mutate == 'quarter' else 1.0)
    v = g * k
    e = U * np.abs(v)
    if mask is not None:
        v, e = _masked(v, e, mask, mask_slope)
    return v, e * WIDEN


def upsample2_bwd(g):
    """gx = (p0 + p1) + (p2 + p3): u per sum."""
    p0, p1, p2, p3 = _quad(g)
    s = (p0 + p1) + (p2 + p3)
    return s, U * (np.abs(p0 + p1) + np.abs(p2 + p3) + np.abs(s)) * WIDEN


def axpby_mask(x, other=None, mask=None, a=1.0, b=0.0, mask_slope=0.2, mutate=None):
    """y = (a x + b other) (mask > 0 ? 1 : slope): u for a x, u for b other, u for the sum, u for the slope."""
    a, b = f32(a), f32(b)
    v = _d(x) * a
    e = U * np.abs(v)
    if other is not None:
        bq = b * (1.05 if mutate == 'b' else 1.0) * _d(other)
        v = v + bq
        e = e + U * np.abs(bq) + U * np.abs(v)
    if mask is not None:
        v, e = _masked(v, e, mask, mask_slope)
    return v, e * WIDEN


# ------------------------------------------------------------------------------------------------------------------- assertion
def ratio(got, want, bound):
    """(max err / bound, flat index of the worst element): 0 where the error is 0, inf where an error meets a bound of 0."""
    got, want, bound = (np.asarray(v, np.float64).reshape(-1) for v in (got, want, bound))
    err = np.abs(got - want)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, 0.0, err / bound)
    i = int(np.argmax(q))
    return float(q[i]), i


# ------------------------------------------------------------------------------------------- shapes and inputs of both tiers
PN_C = (4, 8, 12, 16, 20, 48, 144, 256, 512, 528)        # LPP 1 .. 64, idle lanes (12, 20, 48, 144), one / two / a ragged third float4 per lane
PN_P = (1, 5, 37, 1000)                                  # less than one workgroup's pixels; no multiple of 256 / LPP; several workgroups
PN_WRAP = ((262144 + 37, 20), (16384 + 5, 512))          # the first sizes with P x LPP > 4096 x 256, one per general kernel template shape
MB_CASES = ((1, 4, 16, 16), (3, 3, 16, 512), (2, 4, 16, 512), (2, 5, 16, 512), (2, 3, 16, 36), (1, 1, 16, 4), (2, 17, 16, 8), (1, 5, 64, 8))
POOL_CASES = ((2, 1, 1, 4), (1, 3, 5, 12), (2, 8, 4, 16), (3, 4, 4, 512))            # N, coarse H, coarse W, C
POOL_WRAP_FWD = (1, 520, 512, 16)                        # 1 064 960 coarse float4 (avgpool2_fwd, upsample2_bwd: one thread per coarse float4)
POOL_WRAP_BWD = (1, 260, 256, 16)                        # 1 064 960 fine float4 (avgpool2_bwd: one thread per fine float4)
AXPBY_WRAP = 4 * (1048576 + 3)
SIGNBYTES_WRAP = 2097152 + 5                             # pg_signbytes_to_mask caps its grid at 8192 workgroups


def _randn(seed, *shape):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy()


def pn_inputs(P, C):
    """fp32 x, gy, t, a of a [P, C] PixelNorm case: seeded noise; x[0, 1] = 0.0 and x[0, 2] = -0.0 (so y holds both zeros), and, from
    P = 5 on, pixel P // 2 all zero (r = rsqrt(eps), y = 0, every mask entry takes the slope)."""
    x, gy, t, a = (_randn(1000 * i + P + C, P, C) for i in range(4))
    x[0, 1], x[0, 2] = 0.0, -0.0
    if P >= 5:
        x[P // 2] = 0.0
    return x, gy, t, a


def mb_inputs(G, n, HW, C, cond=False):
    """fp32 x, tx, gy, gy_first of a minibatch-stddev case ([G n, HW, 1, C] and [.., CP], CP = C + 16): seeded noise + 0.3 as the
    older test; every 7th element of x is 0.0 and x[0] is -0.0 (the mask of ``apply_mask``).  ``cond``: x = 30 + 0.01 noise."""
    NB, cp = G * n, C + 16
    seed = 100 * G + 10 * n + HW + C
    x = _randn(seed, NB, HW, 1, C)
    x = (np.float32(30) + np.float32(0.01) * x) if cond else x + np.float32(0.3)
    if not cond:
        x.reshape(-1)[::7] = 0.0
        x.reshape(-1)[0] = -0.0
    return x, _randn(seed + 1, NB, HW, 1, C), _randn(seed + 2, NB, HW, 1, cp), _randn(seed + 3, NB, HW, 1, cp)


def shard_rows(G, n, world):
    """Index lists that cut a batch of G groups of n images into ``world`` shards: shard r holds n / world images of EVERY group."""
    per = n // world
    return [np.concatenate([np.arange(g * n + r * per, g * n + (r + 1) * per) for g in range(G)]) for r in range(world)]


def pool_inputs(N, H, W, C):
    """fp32 fine x [N, 2H, 2W, C], coarse other and gy [N, H, W, C], fine mask with 0.0 and -0.0 among its entries."""
    seed = 1000 * N + 100 * H + 10 * W + C
    x, m = _randn(seed, N, 2 * H, 2 * W, C), _randn(seed + 3, N, 2 * H, 2 * W, C)
    m.reshape(-1)[::5] = 0.0
    m.reshape(-1)[1::10] = -0.0
    return x, _randn(seed + 1, N, H, W, C), _randn(seed + 2, N, H, W, C), m
