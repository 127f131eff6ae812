"""fp64 reference and derived per-element bound for one ``pg_adam`` step (test infrastructure; both tiers hold ``ops.adam`` and
``FusedAdam`` to it: tests/test_optimizer_host.py, tests/test_optimizer_gpu.py).

The kernel (csrc/elementwise.hip, ``adam_kernel``) evaluates, per element and in fp32,

    g_  = g * grad_scale
    m'  = m * beta1 + omb1 * g_                     (beta1 == 0: m is taken as 0 and never read)
    v'  = v * beta2 + (omb2 * g_) * g_
    den = sqrtf(v') * inv_bc2_sqrt + eps
    p'  = p - (step_size * m') / den

with the scalars formed on the host side of the C ABI in fp32: ``step_size = lr / bc1``, ``inv_bc2_sqrt = 1 / bc2_sqrt``,
``omb1 = 1 - beta1``, ``omb2 = 1 - beta2``.  ``reference`` evaluates the same expressions in fp64 with exactly those fp32 scalars, so
that what is left between it and the kernel is the rounding of the per-element operations alone.

Bound.  u = 2^-24 is charged per add, multiply and fma (relative to the magnitude of the rounded result), 2u per sqrtf and per division,
and every charge is propagated to first order (a contracted fma rounds once where the two separate operations charged here round twice,
so the bound covers whatever the compiler contracts):

    e_g   = u |g_|
    e_m   = u |m beta1| + u |omb1 g_| + omb1 e_g + u |m'|
    e_v   = u |v beta2| + 4u omb2 g_^2 + u |v'|            (omb2*g_ and (.)*g_ round once each; e_g enters twice)
    e_s   = 2u s + e_v / (2 s),  s = sqrt(v')              (s == 0 only where v and g are exactly 0: then e_v = 0 and e_s = 0)
    e_den = u |s c| + c e_s + u den,  c = inv_bc2_sqrt
    e_num = u |num| + step_size e_m,  num = step_size m'
    e_q   = 2u |q| + e_num / den + |q| e_den / den,  q = num / den
    e_p   = e_q + u |p'|

The products of two charges that the first-order propagation drops are below 16 u times the bound (fewer than 16 charged operations in
any chain), so every bound is widened by the factor (1 + 2^-20).  No intermediate may be subnormal (relative charges do not hold there):
``reference`` raises if one is; exact zeros are fine.  Nothing here is fitted to an observed error."""
import math

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -20
FLT_MIN = float(np.finfo(np.float32).tiny)


def bias_corrections(t, beta1, beta2):
    """(bc1, bc2_sqrt) of step ``t`` as ``FusedAdam.step`` forms them (Python floats; they become fp32 at the C ABI)."""
    return 1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t)


def scalars(lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale=1.0, exact=False):
    """The kernel's scalar arguments as Python floats: each argument rounded to fp32 where it crosses the C ABI, the derived ones
    formed in fp32 as ``pg_adam`` and ``adam_kernel`` form them.  ``exact=True`` skips every rounding (the host test that ties the
    formulas to ``torch.optim.Adam`` in float64 uses it)."""
    if exact:
        return dict(step_size=lr / bc1, beta1=beta1, beta2=beta2, omb1=1.0 - beta1, omb2=1.0 - beta2, eps=eps,
                    inv_bc2_sqrt=1.0 / bc2_sqrt, grad_scale=grad_scale)
    f = np.float32
    lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale = (f(x) for x in (lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale))
    return dict(step_size=float(lr / bc1), beta1=float(beta1), beta2=float(beta2), omb1=float(f(1) - beta1), omb2=float(f(1) - beta2),
                eps=float(eps), inv_bc2_sqrt=float(f(1) / bc2_sqrt), grad_scale=float(grad_scale))


def _normal(*arrays):
    for a in arrays:
        a = np.abs(a)
        if np.any((a > 0) & (a < FLT_MIN)):
            raise ValueError('emu_adam.reference: a subnormal intermediate; the relative bound does not hold for these operands')


def reference(p, g, m, v, lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale=1.0, exact=False):
    """One step in fp64 on host copies of the fp32 operands: ``(p', m', v', bound_p, bound_m, bound_v)`` (see the module docstring)."""
    k = scalars(lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale, exact)
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    if k['beta1'] == 0.0:
        m = np.zeros_like(g)
    g_ = g * k['grad_scale']
    mb, og = m * k['beta1'], k['omb1'] * g_
    m1 = mb + og
    vb, t2 = v * k['beta2'], k['omb2'] * g_ * g_
    v1 = vb + t2
    s = np.sqrt(v1)
    c = k['inv_bc2_sqrt']
    den = s * c + k['eps']
    num = k['step_size'] * m1
    q = num / den
    p1 = p - q
    _normal(g_, mb, og, m1, vb, k['omb2'] * g_, t2, v1, s * c, num, q, p1)
    e_g = U * np.abs(g_)
    e_m = U * np.abs(mb) + U * np.abs(og) + k['omb1'] * e_g + U * np.abs(m1)
    e_v = U * np.abs(vb) + 4 * U * t2 + U * v1
    with np.errstate(divide='ignore', invalid='ignore'):
        e_s = 2 * U * s + np.where(s > 0, e_v / (2 * s), 0.0)
    e_den = U * s * c + c * e_s + U * den
    e_num = U * np.abs(num) + k['step_size'] * e_m
    e_q = 2 * U * np.abs(q) + e_num / den + np.abs(q) * e_den / den
    e_p = e_q + U * np.abs(p1)
    return p1, m1, v1, e_p * SECOND_ORDER, e_m * SECOND_ORDER, e_v * SECOND_ORDER
