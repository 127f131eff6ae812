"""Selectable GAN objectives: ``gan_losses(kind, penalty=...)`` -> ``(D_loss, G_loss)`` for ``Trainer``.

``kind`` is 'wgan', 'logistic' (non-saturating), 'hinge' or 'lsgan'; ``penalty`` is 'gp' (the WGAN-GP gradient penalty at mixed images),
'r1' ((gamma / 2) |dD/dx|^2 at the real images) or None.  The returned functions have the call signatures of ``wgan_gp_D_loss`` /
``wgan_gp_G_loss`` and return ``LossTensor``s whose ``backward()`` runs the explicit HIP schedules of ``engine``.  The whole step depends
on the objective in its loss block only (csrc/gan_losses.hip): 'gp' and 'r1' run the three-pass schedule of WGAN-GP -- R1 as the
penalty at mixing factors 0, drawing nothing from the mixing-factor stream -- and replay from launch plans of their own; without a
penalty the step is one pass over [real | fake] and runs eagerly.  Both functions are thin closures over the one D and the one G
dispatcher of wgan_gp_loss.py, which WGAN-GP on the original kernels takes too: the objective (``engine.Objective``) is all that differs.

``gan_losses('wgan', penalty='gp')`` with default arguments IS the pair ``(wgan_gp_D_loss, wgan_gp_G_loss)``: Trainer's deferred D
update and early generator pass are keyed to those two objects and stay with them.

``augment=`` an ``augment.Augmenter``: everything D sees goes through it -- reals and fakes in the D step, fakes in the G step, whose
gradient returns through the transpose -- and the pair is ALWAYS a pair of new closures, on the 'pinned' kernels."""
from . import engine, ops, wgan_gp_loss

PENALTIES = ('gp', 'r1', None)


SIGN_KINDS = ('logistic', 'hinge')     # the kinds whose decision boundary is score 0: what plugins.AugmentController may steer by


def gan_losses(kind='wgan', penalty='gp', penalty_weight=10.0, drift=None, gp_target=1.0, augment=None):
    """``(D_loss, G_loss)`` of the objective.  ``penalty_weight``: lambda of 'gp', gamma of 'r1'; ``drift``: weight of the s_r^2 term
    (default 0.001 for 'wgan', 0 otherwise); ``gp_target``: the target norm of 'gp'; ``augment``: an ``augment.Augmenter`` or None.
    ValueError for an unknown name, a non-positive weight or target, a negative drift, an Augmenter with a controller attached under a
    kind whose real scores do not sit around a boundary at 0 ('wgan', 'lsgan': those run with a fixed ``p``)."""
    if kind not in ops.GAN_KINDS:
        raise ValueError('gan_losses: kind %r (one of %s)' % (kind, ', '.join(sorted(ops.GAN_KINDS))))
    if penalty not in PENALTIES:
        raise ValueError("gan_losses: penalty %r ('gp', 'r1' or None)" % (penalty,))
    if drift is None:
        drift = engine.WGAN_GP.drift if kind == 'wgan' else 0.0          # (wgan_gp_D_loss's iwass_epsilon)
    penalty_weight, drift, gp_target = float(penalty_weight), float(drift), float(gp_target)
    if not penalty_weight > 0.0:
        raise ValueError('gan_losses: penalty_weight %r must be positive' % penalty_weight)
    if not gp_target > 0.0:
        raise ValueError('gan_losses: gp_target %r must be positive' % gp_target)
    if not drift >= 0.0:
        raise ValueError('gan_losses: drift %r must not be negative' % drift)
    if augment is None and (kind, drift, penalty, penalty_weight, gp_target) == engine.WGAN_GP[:5]:
        return wgan_gp_loss.wgan_gp_D_loss, wgan_gp_loss.wgan_gp_G_loss
    if augment is not None:
        from .augment import Augmenter
        if not isinstance(augment, Augmenter):
            raise ValueError('gan_losses: augment %r is not an Augmenter' % (augment,))
        if augment.controller is not None and kind not in SIGN_KINDS:
            raise ValueError('gan_losses: the Augmenter is steered by an AugmentController, which reads the sign of the real scores: '
                             "valid for %s, not for %r (run it with a fixed p)" % (' and '.join(SIGN_KINDS), kind))
        augment.kind = kind                                              # (what a controller attached later is checked against)
    obj = engine.Objective(kind, drift, penalty, penalty_weight, gp_target, augment=augment)

    def D_loss(D, G, real_images_in, fake_latents_in, return_all=True):
        return wgan_gp_loss._d_loss(obj, D, G, real_images_in, fake_latents_in, return_all)

    def G_loss(G, D, fake_latents_in):
        return wgan_gp_loss._g_loss(obj, G, D, fake_latents_in)

    D_loss.objective = G_loss.objective = obj
    D_loss.__name__, G_loss.__name__ = '%s_%s_D_loss' % (kind, penalty or 'plain'), '%s_G_loss' % kind
    return D_loss, G_loss
