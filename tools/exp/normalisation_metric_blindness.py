"""What ``max|a-b| / max|b|`` reads when one factor of the minibatch-stddev adjoint is wrong, next to the per-element ``err / bound`` of
tests/norm_ref.py (CPU, float64 evaluation of the contract; docs/experiments_normalisation_tests.md §1).

    python tools/exp/normalisation_metric_blindness.py

Inputs and shapes are those of ``test_mbstd`` in tests/test_kernels_gpu.py, which asserts ``< 2e-5`` on the plain adjoint and ``< 1e-4`` with the
Hessian-vector term; the last line of every case zeroes the pass-through channels of ``gy`` instead."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import norm_ref as ref  # noqa: E402
from conftest import rel_err  # noqa: E402


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g)


def main():
    print('%-14s %-44s %-18s %-10s %s' % ('case (G, n, C)', 'change', 'old metric (mask off / on)', 'old bound', 'new err / bound (the smaller)'))
    for G, n, C in ((1, 4, 16), (2, 5, 32), (3, 3, 512), (3, 16, 512)):
        cp = C + 16
        x = (rnd(G * n, 4, 4, C) + 0.3).numpy()
        tx, gy, gf = rnd(G * n, 4, 4, C, seed=1).numpy(), rnd(G * n, 4, 4, cp, seed=2).numpy(), rnd(G * n, 4, 4, cp, seed=3).numpy()
        _, _, mu, _, sigma, _ = ref.mbstd_fwd(x, G, cp)
        stats = np.stack([mu, sigma], 1)
        ty, e_ty, tmean, _, dot, _ = ref.mbstd_tangent(tx, stats, G, cp, [(x, tx)])
        hv = dict(tx=tx, tstats=np.stack([tmean, dot], 1), gy_first=gf)
        no_std, no_pass = gy.copy(), gy.copy()
        no_std[..., C] = 0
        no_pass[..., :C] = 0
        rows = (('std path dropped', gy, {}, (no_std, {}, None), 2e-5),
                ('std path x 1.05', gy, {}, (gy, {}, 'std'), 2e-5),
                ('hvp dropped (bwd+hvp)', gy, hv, (gy, {}, None), 1e-4),
                ('(x-mu) piece of hvp x 1.05 (hvp only)', None, hv, (None, hv, 'hvp_x'), 1e-4),
                ('(tx-mean) piece of hvp x 1.05 (hvp only)', None, hv, (None, hv, 'hvp_t'), 1e-4),
                ('std path x 1.05, pass-through channels 0', no_pass, {}, (no_pass, {}, 'std'), 2e-5))
        for what, g, kw, (g2, kw2, mutate), old_bound in rows:
            old, new = [], []
            for am in (False, True):
                want, bound = ref.mbstd_bwd(g, x, stats, G, am, 0.2, **kw)
                wrong = ref.mbstd_bwd(g2, x, stats, G, am, 0.2, mutate=mutate, **kw2)[0]
                old.append(rel_err(wrong, want))
                new.append(ref.ratio(wrong, want, bound)[0])
            print('%-14s %-44s %.1e / %.1e  %-10.0e %.1e' % ((G, n, C), what, old[0], old[1], old_bound, min(new)))
        wrong = ty.copy()
        wrong[..., C] *= 1.05
        print('%-14s %-44s %-18.1e %-10.0e %.1e' % ((G, n, C), "tangent's stddev channel x 1.05", rel_err(wrong, ty), 2e-5, ref.ratio(wrong, ty, e_ty)[0]))


if __name__ == '__main__':
    main()
