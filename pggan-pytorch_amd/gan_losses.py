"""Selectable GAN objectives: ``gan_losses(kind, penalty=...)`` -> ``(D_loss, G_loss)`` for ``Trainer``.

``kind`` is 'wgan', 'logistic' (non-saturating), 'hinge' or 'lsgan'; ``penalty`` is 'gp' (the WGAN-GP gradient penalty at mixed images),
'r1' ((gamma / 2) |dD/dx|^2 at the real images) or None.  The returned functions have the call signatures of ``wgan_gp_D_loss`` /
``wgan_gp_G_loss`` and return ``LossTensor``s whose ``backward()`` runs the explicit HIP schedules of ``engine``.  The whole step depends
on the objective in its loss block only (csrc/gan_losses.hip): 'gp' and 'r1' run the three-pass schedule of WGAN-GP -- R1 as the
penalty at mixing factors 0, drawing nothing from the mixing-factor stream -- and replay from launch plans of their own; without a
penalty the step is one pass over [real | fake] and runs eagerly (``engine.d_plain_loss_forward``).

``gan_losses('wgan', penalty='gp')`` with default arguments IS the pair ``(wgan_gp_D_loss, wgan_gp_G_loss)``: Trainer's deferred D
update and early generator pass are keyed to those two objects and stay with them."""
import torch

from . import engine, ops, wgan_gp_loss
from .wgan_gp_loss import LossTensor

PENALTIES = ('gp', 'r1', None)
_WGAN_DRIFT = 0.001            # wgan_gp_D_loss's iwass_epsilon
_zero_mix = {}                 # (n, device) -> [n, 1] zeros: the mixing factors of R1 (read only)


def _zeros(n, device):
    key = (n, str(device))
    if key not in _zero_mix:
        _zero_mix[key] = torch.zeros((n, 1), device=device, dtype=torch.float32)
    return _zero_mix[key]


def gan_losses(kind='wgan', penalty='gp', penalty_weight=10.0, drift=None, gp_target=1.0):
    """``(D_loss, G_loss)`` of the objective.  ``penalty_weight``: lambda of 'gp', gamma of 'r1'; ``drift``: weight of the s_r^2 term
    (default 0.001 for 'wgan', 0 otherwise); ``gp_target``: the target norm of 'gp'.  ValueError for an unknown name, a non-positive
    weight or target, a negative drift."""
    if kind not in ops.GAN_KINDS:
        raise ValueError('gan_losses: kind %r (one of %s)' % (kind, ', '.join(sorted(ops.GAN_KINDS))))
    if penalty not in PENALTIES:
        raise ValueError("gan_losses: penalty %r ('gp', 'r1' or None)" % (penalty,))
    if drift is None:
        drift = _WGAN_DRIFT if kind == 'wgan' else 0.0
    penalty_weight, drift, gp_target = float(penalty_weight), float(drift), float(gp_target)
    if not penalty_weight > 0.0:
        raise ValueError('gan_losses: penalty_weight %r must be positive' % penalty_weight)
    if not gp_target > 0.0:
        raise ValueError('gan_losses: gp_target %r must be positive' % gp_target)
    if not drift >= 0.0:
        raise ValueError('gan_losses: drift %r must not be negative' % drift)
    if (kind, penalty, penalty_weight, drift, gp_target) == ('wgan', 'gp', 10.0, _WGAN_DRIFT, 1.0):
        return wgan_gp_loss.wgan_gp_D_loss, wgan_gp_loss.wgan_gp_G_loss
    obj = engine.Objective(kind, drift, penalty, penalty_weight, gp_target)

    def D_loss(D, G, real_images_in, fake_latents_in, return_all=True):
        D.zero_grad()
        G.zero_grad()
        n = real_images_in.size(0)
        if penalty is None:
            d_cost, d_real_loss, d_fake_loss, state = engine.d_plain_loss_forward(D, G, real_images_in, fake_latents_in, obj)
            d_cost = LossTensor.wrap(d_cost, lambda scale: engine.d_plain_loss_backward(state, scale))
            return (d_cost, d_real_loss, d_fake_loss) if return_all else d_cost
        if penalty == 'r1':
            mix = _zeros(n, real_images_in.device)                           # (the mixing-factor stream is not touched)
        elif wgan_gp_loss.mixing_factors is not None:
            mix = wgan_gp_loss.mixing_factors.to(device=real_images_in.device, dtype=torch.float32).reshape(n, 1)
            wgan_gp_loss.mixing_factors = None
        else:
            mix = wgan_gp_loss._draw_mixing_factors(n, real_images_in.device)
        mode = wgan_gp_loss._replay_mode(D) if (float(D.alpha) >= 1.0 and real_images_in.is_cuda and hasattr(D, '_flat_param')
                                                and D._rt.global_stddev is None) else None
        if mode == 'plan' and wgan_gp_loss._exchange_instrumented(D):
            mode = None
        if mode is not None:
            from . import graphs, plans
            real_c = engine._check_dev(real_images_in, 'real images')
            z_c = engine._check_dev(fake_latents_in, 'latents')
            # (the objective carries its own hyper-parameters: the three WGAN-GP slots of the key are left at 0)
            losses = (graphs if mode == 'graph' else plans).d_step(D, G, real_c, z_c, mix.contiguous(), 0.0, 0.0, 0.0, obj)
            d_cost = LossTensor.wrap(losses[0], wgan_gp_loss._replayed_backward(D))
            return (d_cost, losses[1], losses[2]) if return_all else d_cost
        d_cost, d_real_loss, d_fake_loss, state = engine.d_loss_forward(D, G, real_images_in, fake_latents_in, mix, 0.0, 0.0, 0.0, obj)
        d_cost = LossTensor.wrap(d_cost, lambda scale: engine.d_loss_backward(state, scale))
        return (d_cost, d_real_loss, d_fake_loss) if return_all else d_cost

    def G_loss(G, D, fake_latents_in):
        G.zero_grad()
        mode = wgan_gp_loss._replay_mode(G) if (float(G.alpha) >= 1.0 and fake_latents_in.is_cuda and hasattr(G, '_flat_param')
                                                and D._rt.global_stddev is None) else None
        if mode == 'plan' and wgan_gp_loss._exchange_instrumented(G):
            mode = None
        if mode is not None:
            from . import graphs, plans
            g_cost = (graphs if mode == 'graph' else plans).g_step(G, D, engine._check_dev(fake_latents_in, 'latents'), obj)
            return LossTensor.wrap(g_cost, wgan_gp_loss._replayed_backward(G))
        g_cost, state = engine.g_loss_forward(G, D, fake_latents_in, obj)
        return LossTensor.wrap(g_cost, lambda scale: engine.g_loss_backward(state, scale))

    D_loss.objective = G_loss.objective = obj
    D_loss.__name__, G_loss.__name__ = '%s_%s_D_loss' % (kind, penalty or 'plain'), '%s_G_loss' % kind
    return D_loss, G_loss
