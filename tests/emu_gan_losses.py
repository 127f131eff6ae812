"""torch-CPU statements of ``ops.gan_d_loss`` / ``ops.gan_g_loss`` / ``ops.r1_seed`` (include/pggan_hip_gan.h) for the
host tests: tests/test_gan_losses_host.py installs them onto ``emu_ops`` the way tests/test_ema_host.py installs ``emu_ema``.  Test
infrastructure only; the kernels themselves are held to tests/gan_losses_ref.py on the GPU."""
import torch

KINDS = ('wgan', 'logistic', 'hinge', 'lsgan')


def _softplus(x):
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def _sigmoid(x):
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, torch.ones_like(e), e) / (1 + e)


def _term(kind, s, fake):
    """(term, derivative): F for ``fake``, otherwise R without the drift term."""
    if kind == 'wgan':
        return (s.clone(), torch.ones_like(s)) if fake else (-s, -torch.ones_like(s))
    if kind == 'logistic':
        x = s if fake else -s
        return _softplus(x), (_sigmoid(x) if fake else -_sigmoid(x))
    if kind == 'hinge':
        if fake:
            return (1 + s).clamp(min=0), (s > -1).to(s.dtype)
        return (1 - s).clamp(min=0), -(s < 1).to(s.dtype)
    if kind == 'lsgan':
        t = s if fake else s - 1
        return t * t, 2 * t
    raise KeyError(kind)


def gan_d_loss(scores, pen, N, kind, drift):
    groups = scores.numel() // N
    sr, sf = scores[:N], scores[N:2 * N]
    r, dr = _term(kind, sr, False)
    f, df = _term(kind, sf, True)
    r = r + sr * sr * drift
    dr = dr + 2 * drift * sr
    t = f + r if pen is None else f + r + pen
    gscore = torch.cat([dr / N, df / N] + ([torch.zeros(N, dtype=scores.dtype)] if groups == 3 else []))
    return t.mean(), r.view(N, 1).clone(), f.view(N, 1).clone(), gscore


def gan_g_loss(scores, kind):
    N = scores.shape[0]
    l, dl = _term('wgan' if kind == 'hinge' else kind, scores, False)
    return l.mean(), dl / N


def r1_seed(g, ss, gamma, inv_n):
    return 0.5 * gamma * ss, g * (inv_n * gamma)
