"""TEST INFRASTRUCTURE: float64 twins of the latent projection (pggan-pytorch_amd/projection.py, include/pggan_hip_projection.h).  CPU only.

``pyramid_loss_ref`` is the definition of the loss and its closed-form gradient; ``pyramid_loss_torch`` is the same loss written with
torch ops so that autograd can differentiate it (tests/test_projection_host.py holds the closed form to it, and the dz tests chain it
behind ``oracle.generator_forward``); ``project_ref`` is the search: the oracle generator, autograd on z, the Adam arithmetic of
pg_adam and the projector's cosine schedule, in the dtype of its arguments."""
import math

import torch
import torch.nn.functional as F


def levels(r):
    """Levels of the pyramid of an r x r image: sides r, r/2, .., 4."""
    return int(r).bit_length() - 2


def _weights(weights, r):
    L = levels(r)
    if weights is None:
        return [1.0] * L
    w = [float(x) for x in weights]
    assert 1 <= len(w) <= L
    return w + [0.0] * (L - len(w))


def pyramid_terms_ref(img, target, weights=None):
    """Per level l: (w_l mean_{c,y,x} P_l(e)^2 [N],  w_l 2 / (C r_l^2) 4^-l P_l(e)[.., y >> l, x >> l] [N,C,r,r]) in float64."""
    e = img.double() - target.double()
    N, C, r, _ = e.shape
    out, p = [], e
    for l, w in enumerate(_weights(weights, r)):
        rl = r >> l
        loss = w * (p * p).mean(dim=(1, 2, 3))
        up = p.repeat_interleave(1 << l, dim=2).repeat_interleave(1 << l, dim=3)
        out.append((loss, (w * 2.0 / (C * rl * rl) / 4.0 ** l) * up))
        p = F.avg_pool2d(p, 2) if rl > 4 else None
    return out


def pyramid_loss_ref(img, target, weights=None):
    """(loss [N], grad [N,C,r,r]) of the definition, float64: the closed-form gradient, no autograd."""
    terms = pyramid_terms_ref(img, target, weights)
    return sum(t[0] for t in terms), sum(t[1] for t in terms)


def pyramid_bounds_ref(img, target, weights=None):
    """(sum_l w_l mean P_l(e)^2 [N],  sum_l |term_l| [N,C,r,r]): the magnitudes one fp32 rounding of each output is charged against."""
    terms = pyramid_terms_ref(img, target, weights)
    return sum(t[0].abs() for t in terms), sum(t[1].abs() for t in terms)


def pyramid_loss_torch(img, target, weights=None):
    """The loss [N] in the dtype of ``img``, differentiable."""
    e = img - target
    r = e.shape[-1]
    total, p = 0.0, e
    for l, w in enumerate(_weights(weights, r)):
        if w != 0.0:
            total = total + w * (p * p).mean(dim=(1, 2, 3))
        if (r >> l) > 4:
            p = F.avg_pool2d(p, 2)
    return total


def loss_and_dz_ref(oracle, params, cfg, z, targets, depth, alpha, weights=None, signs=None):
    """(loss [N], dz [N,latent], forced_signs object or None) of the oracle generator + the twin loss in the dtype of ``params`` / ``z``;
    ``signs``: evaluate on that linear piece (``oracle.forced_signs``)."""
    z = z.detach().clone().requires_grad_(True)
    fs = None
    if signs is None:
        img = oracle.generator_forward(params, cfg, z, depth, alpha)
    else:
        with oracle.forced_signs(signs) as fs:
            img = oracle.generator_forward(params, cfg, z, depth, alpha)
    loss = pyramid_loss_torch(img, targets.to(img.dtype), weights)
    dz, = torch.autograd.grad(loss.sum(), z)
    return loss.detach(), dz, fs


def project_ref(oracle, params, cfg, targets, z0, steps, lr, betas, depth, alpha, weights=None, eps=1e-8):
    """The search of ``Projector.project`` in the dtype of ``params`` / ``z0``: returns (z [N,latent], history [steps,N] of the loss
    before every step, final loss [N]).  Adam as pg_adam: p -= lr_t / bc1 * m / (sqrt(v) / sqrt(bc2) + eps), lr_t = lr (1 + cos(pi t /
    steps)) / 2."""
    z = z0.detach().clone()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    b1, b2 = betas
    history = []
    for t in range(steps):
        loss, dz, _ = loss_and_dz_ref(oracle, params, cfg, z, targets, depth, alpha, weights)
        history.append(loss)
        m = b1 * m + (1.0 - b1) * dz
        v = b2 * v + (1.0 - b2) * dz * dz
        lr_t = lr * 0.5 * (1.0 + math.cos(math.pi * t / steps))
        bc1, bc2_sqrt = 1.0 - b1 ** (t + 1), math.sqrt(1.0 - b2 ** (t + 1))
        z = z - (lr_t / bc1) * m / (v.sqrt() / bc2_sqrt + eps)
    with torch.no_grad():
        final = pyramid_loss_torch(oracle.generator_forward(params, cfg, z, depth, alpha), targets.to(z.dtype), weights)
    return z, torch.stack(history), final
