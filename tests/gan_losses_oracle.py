"""The selectable objectives of DESIGN.md section 7 as float64 torch autograd through ``oracle.discriminator_forward`` /
``oracle.generator_forward`` (test infrastructure shared by tests/test_gan_losses_host.py and tests/test_gan_losses_gpu.py): the table's
expressions written once, with torch's own subgradients (``relu`` is 0 at the kink)."""
from collections import OrderedDict

import torch

from oracle import pggan_cpu as oc


def softplus(x):
    """torch's own softplus, whose derivative is the sigmoid everywhere (autograd through ``max(x, 0) + log1p(exp(-|x|))`` would take
    the subgradients of ``max`` and ``abs`` at x = 0 and return 1 there instead of 1/2).  Above the threshold torch returns x itself:
    at 50 that is e^-50 = 2e-22 away from the function."""
    return torch.nn.functional.softplus(x, beta=1.0, threshold=50.0)


def real_term(kind, s):
    """R[n] without the drift term; also L[n] of every kind but 'hinge'."""
    return {'wgan': lambda: -s, 'logistic': lambda: softplus(-s), 'hinge': lambda: torch.relu(1 - s), 'lsgan': lambda: (s - 1) ** 2}[kind]()


def fake_term(kind, s):
    return {'wgan': lambda: s, 'logistic': lambda: softplus(s), 'hinge': lambda: torch.relu(1 + s), 'lsgan': lambda: s ** 2}[kind]()


def generator_term(kind, s):
    return -s if kind == 'hinge' else real_term(kind, s)


def to64(params):
    return OrderedDict((k, v.double() if torch.is_tensor(v) else v) for k, v in params.items())


def _grads(cost, p):
    names = oc.tensor_names(p)
    gr = torch.autograd.grad(cost, [p[k] for k in names], allow_unused=True)
    return OrderedDict((k, g) for k, g in zip(names, gr) if g is not None)


def d_loss_and_grads(dparams, gparams, cfg, real, latents, mix, depth, alpha, kind, drift, penalty, weight, target=1.0):
    """dict(d_cost, R [N,1], F [N,1], s_r, s_f, grads) in float64.  ``mix`` [N,1] is read by 'gp' only."""
    dp, gp = oc._leafify(to64(dparams)), to64(gparams)
    real, latents = real.double(), latents.double()
    n = real.size(0)
    s_r = oc.discriminator_forward(dp, cfg, real, depth, alpha)
    with torch.no_grad():
        fake = oc.generator_forward(gp, cfg, latents, depth, alpha)
    s_f = oc.discriminator_forward(dp, cfg, fake, depth, alpha)
    R = real_term(kind, s_r) + drift * s_r ** 2
    F = fake_term(kind, s_f)
    total = F + R
    if penalty == 'gp':
        total = total + oc.gradient_penalty(dp, cfg, real, fake, mix.double(), depth, alpha, weight, target).view(n, 1)
    elif penalty == 'r1':
        x = real.detach().requires_grad_(True)
        scores = oc.discriminator_forward(dp, cfg, x, depth, alpha)
        g = torch.autograd.grad(scores.sum(), x, create_graph=True)[0]
        total = total + (0.5 * weight) * g.reshape(n, -1).pow(2).sum(1).view(n, 1)
    else:
        assert penalty is None
    d_cost = total.mean()
    gs = torch.autograd.grad(d_cost, [s_r, s_f], retain_graph=True)
    return dict(d_cost=d_cost.detach(), R=R.detach(), F=F.detach(), s_r=s_r.detach(), s_f=s_f.detach(), grads=_grads(d_cost, dp),
                bias_terms=float(sum(g.abs().sum() for g in gs)))


def grad_err(name, mine, want, bias_terms=None):
    """``conftest.rel_err`` (max |a - b| / max |b|) of one gradient tensor -- except where that metric is undefined: the gradient of
    D's ``linear.bias`` is sum_n d cost / d score[n], and it is EXACTLY zero whenever every term of an objective is on a linear piece
    (hinge with all scores inside the margins: N times -1/N plus N times 1/N), while fp32 adds 2N multiples of fl(1/N) to a few 2^-24
    (N = 3).  Then, and only then (|reference| below 1e-12 of the terms' magnitudes), the error is taken relative to
    ``bias_terms`` = sum_n |d cost / d score[n]|, the magnitude of what was summed."""
    from conftest import rel_err
    if name == 'linear.bias' and bias_terms is not None and float(want.abs().max()) <= 1e-12 * bias_terms:
        return float(mine.detach().cpu().double().abs().max()) / bias_terms
    return rel_err(mine, want)


def g_loss_and_grads(gparams, dparams, cfg, latents, depth, alpha, kind):
    gp, dp = oc._leafify(to64(gparams)), to64(dparams)
    s = oc.discriminator_forward(dp, cfg, oc.generator_forward(gp, cfg, latents.double(), depth, alpha), depth, alpha)
    g_cost = generator_term(kind, s).mean()
    return dict(g_cost=g_cost.detach(), s=s.detach(), grads=_grads(g_cost, gp))
