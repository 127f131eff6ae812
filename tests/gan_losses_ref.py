"""fp64 references and derived per-element bounds for the loss block of the selectable GAN objectives (``pg_gan_d_loss``,
``pg_gan_g_loss``, ``pg_r1_seed``; include/pggan_hip_gan.h), in the style of tests/lossblock_ref.py (test
infrastructure: tests/test_gan_losses_gpu.py holds the kernels to them, tests/test_gan_losses_host.py ties them to float64 autograd of
the table's expressions).

Every reference takes host copies of the fp32 operands, rounds the scalar arguments to fp32 as the C ABI does, forms the derived scalars
the host side of the launch forms in fp32 (``0.5 gamma``, ``inv_n gamma``: operands of the kernel, exact) and evaluates everything else in
fp64.  Every bound follows the operation sequence of csrc/gan_losses.hip, which spells each operation with a rounding intrinsic:
u = 2^-24 relative per add and multiply, 2u per division, propagated to first order; a sum is charged (longest chain of additions a
term passes through) x u x (sum of the terms' magnitudes); the longest chain here has ceil(100 014 / 64) + 6 = 1569 additions (2^-13.4
relative), so every bound is widened by (1 + 2^-12) for the dropped products of charges.

``expf`` and ``log1pf``: no statement of their maximum error ships with the ROCm installation, so
softplus and its derivative were MEASURED on the device against this file's fp64 values over the fixed score set plus 131 058 uniform
scores in [-30, 30] (tools/gan_loss_ulps.py; docs/experiments_gan_losses.md holds the figures) and four times the largest error found, in
units in the last place of the result, is what is charged here (SOFTPLUS_ULPS, SIGMOID_ULPS): the sample is not exhaustive.  A result that
may be subnormal (softplus(-100), the logistic derivative far out) gets an absolute floor of one smallest normal fp32 on top.  Nothing
else is fitted to an observed error."""
import numpy as np

U = 2.0 ** -24
WIDEN = 1.0 + 2.0 ** -12
TINY = float(np.finfo(np.float32).tiny)          # the smallest normal fp32: floor of a result that may be subnormal

KINDS = ('wgan', 'logistic', 'hinge', 'lsgan')
# measured maxima (docs/experiments_gan_losses.md section 1): softplus 1.433 ulp, its derivative 2.049 ulp; rounded up, charged four times
MEASURED_SOFTPLUS_ULPS = 1.44
MEASURED_SIGMOID_ULPS = 2.05
SOFTPLUS_ULPS = 4 * MEASURED_SOFTPLUS_ULPS
SIGMOID_ULPS = 4 * MEASURED_SIGMOID_ULPS

# the fixed score set of the issue: +-0, +-1, the fp32 neighbours of +-1, +-30, +-100, +-1e4
_one = np.float32(1)
FIXED_SCORES = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(_one, np.float32(2)), np.nextafter(_one, np.float32(0)),
                         np.nextafter(-_one, np.float32(-2)), np.nextafter(-_one, np.float32(0)), 30.0, -30.0, 100.0, -100.0, 1e4, -1e4],
                        np.float32)


def f32(x):
    return float(np.float32(x))


def _d(x):
    return np.asarray(x, np.float64)


def ulp32(x):
    """Unit in the last place of the fp32 number nearest to |x| (fp64 in, fp64 out); at least the subnormal spacing."""
    return np.spacing(np.abs(_d(x)).astype(np.float32)).astype(np.float64)


def softplus(x):
    """max(x, 0) + log1p(exp(-|x|)) in fp64."""
    x = _d(x)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    """1 / (1 + e^-x) for x >= 0, e^x / (1 + e^x) for x < 0, in fp64."""
    x = _d(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


def score_term(kind, s, fake):
    """(term, bound, derivative, bound) of one side of the table: ``fake`` selects F[n], otherwise R[n] without the drift term, which is
    L[n] too except for 'hinge' (whose generator term is the 'wgan' one).

    wgan      a copy / a negation, +-1: exact.
    hinge     max(0, 1 -+ s): one addition (u); the derivative is a comparison of the operand itself: exact, 0 AT the kink.
    lsgan     real: t = s - 1 (u), t t (u) -> 2 |t| e_t + u t^2, derivative 2 t -> 2 e_t (the doubling is exact);  fake: s s (u), 2 s exact.
    logistic  softplus(+-s) and +-sigmoid(+-s): SOFTPLUS_ULPS / SIGMOID_ULPS units in the last place of the result + TINY (measured)."""
    s = _d(s)
    zero = np.zeros_like(s)
    if kind == 'wgan':
        return (s.copy(), zero, np.ones_like(s), zero) if fake else (-s, zero, -np.ones_like(s), zero)
    if kind == 'hinge':
        if fake:
            t = np.maximum(0.0, 1.0 + s)
            return t, U * np.abs(1.0 + s), (s > -1.0).astype(np.float64), zero
        t = np.maximum(0.0, 1.0 - s)
        return t, U * np.abs(1.0 - s), -(s < 1.0).astype(np.float64), zero
    if kind == 'lsgan':
        if fake:
            return s * s, U * s * s, 2.0 * s, zero
        t = s - 1.0
        e_t = U * np.abs(t)
        return t * t, 2 * np.abs(t) * e_t + U * t * t, 2.0 * t, 2 * e_t
    if kind == 'logistic':
        x = s if fake else -s
        sp, sg = softplus(x), sigmoid(x)
        return sp, SOFTPLUS_ULPS * ulp32(sp) + TINY, (sg if fake else -sg), SIGMOID_ULPS * ulp32(sg) + TINY
    raise ValueError(kind)


def _chain(N):
    return -(-N // 64) + 6            # one lane adds ceil(N / 64) terms in ascending n, then 6 butterfly levels


def gan_d_loss(s, pen, N, groups, kind, drift):
    """scores s = [real(N) | fake(N) | (mixed(N))], pen [N] or None -> dict name -> (value, bound) for d_cost, d_real, d_fake, gscore
    (``groups`` N entries, the last third 0).

    R = term + (sr sr) drift: the square (u), x drift (u), the sum (u), and the term's own bound.  dR = dterm + (2 drift) sr: x sr (u),
    the sum (u); 2 drift is exact.  gscore = d invn: invn = fl(1 / N) (2u), the product (u).
    d_cost = invn sum_n ((F + R) [+ pen]): each term carries its parts' bounds and one addition each; the chain of ``_chain``; x invn (3u)."""
    drift = f32(drift)
    s = _d(s)
    sr, sf = s[:N], s[N:2 * N]
    r0, e_r0, dr0, e_dr0 = score_term(kind, sr, False)
    f, e_f, df, e_df = score_term(kind, sf, True)
    sq = sr * sr * drift
    r = r0 + sq
    e_r = e_r0 + 2 * U * np.abs(sq) + U * np.abs(r)
    lin = 2.0 * drift * sr
    dr = dr0 + lin
    e_dr = e_dr0 + U * np.abs(lin) + U * np.abs(dr)
    t = f + r
    e_t = e_f + e_r + U * np.abs(t)
    if pen is not None:
        t = t + _d(pen)
        e_t = e_t + U * np.abs(t)
    d_cost = t.sum() / N
    e_cost = (e_t.sum() + _chain(N) * U * np.abs(t).sum()) / N + 3 * U * abs(d_cost)
    gs = [dr / N, df / N] + ([np.zeros(N)] if groups == 3 else [])
    e_gs = [e_dr / N + 3 * U * np.abs(dr) / N, e_df / N + 3 * U * np.abs(df) / N] + ([np.zeros(N)] if groups == 3 else [])
    return dict(d_cost=(d_cost, e_cost * WIDEN), d_real=(r, e_r * WIDEN), d_fake=(f, e_f * WIDEN),
                gscore=(np.concatenate(gs), np.concatenate(e_gs) * WIDEN))


def gan_g_loss(s, kind):
    """(g_cost, bound, gscore, bound): L = the real side's term at s = D(G(z)) ('hinge': -s), the reduction of ``gan_d_loss``."""
    s = _d(s)
    N = s.shape[0]
    l, e_l, dl, e_dl = score_term('wgan' if kind == 'hinge' else kind, s, False)
    g_cost = l.sum() / N
    e_cost = (e_l.sum() + _chain(N) * U * np.abs(l).sum()) / N + 3 * U * abs(g_cost)
    return g_cost, e_cost * WIDEN, dl / N, (e_dl / N + 3 * U * np.abs(dl) / N) * WIDEN


def r1_seed(g, ss, gamma, inv_n):
    """pen[n] = (0.5 gamma) ss[n], u = (inv_n gamma) g: the two coefficients are formed in fp32 by the host side of the launch and are
    operands here, so each result carries one product (u) -- against the DEFINITION (gamma / 2) ss and inv_n gamma g the coefficient of
    u carries one more u (0.5 gamma is exact).  ``ss`` is an operand."""
    N = g.shape[0]
    gamma, inv_n = f32(gamma), f32(inv_n)
    g, ss = _d(g).reshape(N, -1), _d(ss)
    pen = 0.5 * gamma * ss
    u = inv_n * gamma * g
    return pen, U * np.abs(pen) * WIDEN, u, 2 * U * np.abs(u) * WIDEN
