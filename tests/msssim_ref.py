"""The multi-scale structural similarity between image pairs (Wang, Simoncelli & Bovik 2003, in the form Karras et al. 2018 use to detect
loss of variation), stated for the CPU in plain torch.  The dtype follows the input: float32 mirrors the
device's quantisation step operation for operation, float64 is the adjudicator for everything else."""
import math

import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WINDOW, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def scales(resolution):
    """(sides, weights): S = min(5, log2(R) - 3) scales, every side >= 16; the first S published weights over their sum."""
    if resolution < 16 or resolution & (resolution - 1):
        raise ValueError('resolution must be a power of two >= 16')
    S = min(5, int(math.log2(resolution)) - 3)
    total = sum(WEIGHTS[:S])
    return [resolution >> s for s in range(S)], [w / total for w in WEIGHTS[:S]]


def taps(dtype):
    """The 1-D Gaussian taps, normalised to sum 1 in float64, then cast."""
    g = torch.exp(-(torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2) ** 2 / (2 * SIGMA ** 2))
    return (g / g.sum()).to(dtype)


def quantise(x, drange=(-1, 1), quantize=True):
    """(x - lo) * (255 / (hi - lo)) in x's dtype, one rounding per operation; then round half to even and clip to [0, 255]."""
    lo, hi = float(drange[0]), float(drange[1])
    y = (x - torch.tensor(lo, dtype=x.dtype)) * torch.tensor(255.0 / (hi - lo), dtype=x.dtype)
    return y.round().clamp(0, 255) if quantize else y


def pool(x):
    """2x2 box mean, summed ((p00 + p01) + p10) + p11, then x 0.25."""
    return (((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + x[..., 1::2, 0::2]) + x[..., 1::2, 1::2]) * 0.25


def _filter(x):
    """'valid' 11x11 Gaussian of every plane of [n,C,s,s], as a row pass then a column pass."""
    n, C, s, _ = x.shape
    g = taps(x.dtype)
    y = F.conv2d(x.reshape(n * C, 1, s, s), g.view(1, 1, 1, WINDOW))
    return F.conv2d(y, g.view(1, 1, WINDOW, 1)).reshape(n, C, s - WINDOW + 1, s - WINDOW + 1)


def ssim_maps(a, b):
    """(ssim map, cs map) of two [n,C,s,s] batches in [0, 255] units: [n,C,s-10,s-10] each."""
    mu_a, mu_b = _filter(a), _filter(b)
    s_aa = _filter(a * a) - mu_a * mu_a
    s_bb = _filter(b * b) - mu_b * mu_b
    s_ab = _filter(a * b) - mu_a * mu_b
    cs = (2 * s_ab + C2) / (s_aa + s_bb + C2)
    return (2 * mu_a * mu_b + C1) / (mu_a * mu_a + mu_b * mu_b + C1) * cs, cs


def msssim_pairs(a, b, drange=(-1, 1), quantize=True, return_pooled=False):
    """(values [n], terms [n,S]) of the pairs (a[i], b[i]) of two [n,C,R,R] batches; terms = mean cs of every scale below the last and
    mean ssim of the last, over positions and channels; values = prod_s max(terms[s], 0) ^ w_s.  ``return_pooled``: also the list of
    the (a, b) images of every scale below the finest."""
    sides, weights = scales(a.shape[-1])
    a, b = quantise(a, drange, quantize), quantise(b, drange, quantize)
    terms, pooled = [], []
    for s in range(len(sides)):
        ssim, cs = ssim_maps(a, b)
        terms.append((ssim if s == len(sides) - 1 else cs).mean(dim=(1, 2, 3)))
        if s < len(sides) - 1:
            a, b = pool(a), pool(b)
            pooled.append((a, b))
    terms = torch.stack(terms, dim=1)
    values = torch.ones_like(terms[:, 0])
    for s, w in enumerate(weights):
        values = values * terms[:, s].clamp(min=0) ** w
    return (values, terms, pooled) if return_pooled else (values, terms)


def summary(values):
    """(mean, population standard deviation) of the per-pair values, in float64."""
    v = values.double()
    return float(v.mean()), float((v - v.mean()).pow(2).mean().sqrt())
