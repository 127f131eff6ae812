#!/usr/bin/env python
"""Largest error of softplus and of its derivative as csrc/gan_losses.hip evaluates them (``expf`` / ``log1pf`` of the device library), in
units in the last place of the result, against the fp64 values of tests/gan_losses_ref.py.

    python tools/gan_loss_ulps.py

Scores: the fixed set of the tests (+-0, +-1 and their fp32 neighbours, +-30, +-100, +-1e4) plus 131 058 uniform draws in [-30, 30], as
two launches of ``pg_gan_d_loss`` ('logistic', drift 0, no penalty) with N = 65 536 real and as many fake scores: 1 / N is a power of
two, so d_real = softplus(-s_r), d_fake = softplus(s_f) and N x gscore = -+sigmoid(-+s) are the device functions' own values, nothing
else rounded.  Results below the smallest normal fp32 are left out (the tests give those an absolute floor instead).  Four times the
two maxima printed here are SOFTPLUS_ULPS / SIGMOID_ULPS of tests/gan_losses_ref.py.  Needs a GPU."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, 'tests')]


def main():
    import torch
    if not torch.cuda.is_available():
        sys.exit('gan_loss_ulps.py needs a GPU')
    import gan_losses_ref as ref
    import pggan_amd as pg
    N = 65536
    rs = np.random.RandomState(20)
    s = rs.uniform(-30.0, 30.0, 2 * N).astype(np.float32)
    s[:ref.FIXED_SCORES.size] = ref.FIXED_SCORES
    worst = {'softplus': (0.0, 0.0), 'sigmoid': (0.0, 0.0)}
    for half in (s[:N], s[N:]):
        both = np.concatenate([half, half])                       # the same scores as real and as fake: softplus / sigmoid at -s and at s
        _, R, F, gs = pg.ops.gan_d_loss(torch.from_numpy(both).cuda(), None, N, 'logistic', 0.0)
        R, F, gs = (t.cpu().numpy().astype(np.float64).reshape(-1) for t in (R, F, gs))
        x = np.concatenate([-half, half]).astype(np.float64)
        for name, got, want in (('softplus', np.concatenate([R, F]), ref.softplus(x)),
                                ('sigmoid', np.concatenate([-gs[:N], gs[N:]]) * N, ref.sigmoid(x))):
            keep = want >= ref.TINY
            ulps = np.abs(got - want)[keep] / ref.ulp32(want[keep])
            i = int(np.argmax(ulps))
            if ulps[i] > worst[name][0]:
                worst[name] = (float(ulps[i]), float(x[keep][i]))
    for name, (u, at) in worst.items():
        print('[gan_loss_ulps] %-8s largest error %.3f ulp at x = %r  (over %d scores)' % (name, u, at, 4 * N))
    print(json.dumps({k: {'ulps': v[0], 'at': v[1]} for k, v in worst.items()}))


if __name__ == '__main__':
    main()
