"""What the rel. max-norm checks on WEIGHTS read when the optimizer step is wrong (CPU, tests/emu_ops.py; docs/experiments_optimizer_tests.md §1).

    python tools/exp/optimizer_metric_blindness.py unit      # the Adam / d_loss lines of test_linear_gp_loss_adam with one scalar changed
    python tools/exp/optimizer_metric_blindness.py trace     # the trace16 run with the step switched off / scaled by 1.01 and 1.02
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import emu_ops as E  # noqa: E402
from conftest import rel_err  # noqa: E402


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g)


def unit():
    n = 1003
    base = dict(lr=1e-3, beta1=0.0, beta2=0.99, eps=1e-8, bc1=1.0, bc2_sqrt=0.3, grad_scale=0.5)

    def run(**change):
        p, g, m, v = rnd(n), rnd(n, seed=1), rnd(n, seed=2) * 0.1, rnd(n, seed=3).abs() * 0.1
        k = dict(base, **change)
        E.adam(p, g, m, v, k['lr'], k['beta1'], k['beta2'], k['eps'], k['bc1'], k['bc2_sqrt'], k['grad_scale'])
        return p
    want = run()
    step = (want - rnd(n)).abs()
    print('weights max %.2f, step max %.1e median %.1e' % (float(want.abs().max()), float(step.max()), float(step.median())))
    for what, change in (('lr x 1.02', dict(lr=1.02e-3)), ('bc2_sqrt 0.31 for 0.30', dict(bc2_sqrt=0.31)), ('eps 1e-4', dict(eps=1e-4)),
                         ('eps 0', dict(eps=0.0))):
        print('%-28s rel_err of p %.2e   (the test asserts < 2e-5)' % (what, rel_err(run(**change), want)))
    sc, gp = rnd(12, seed=7), torch.rand(4, generator=torch.Generator().manual_seed(0))
    print('%-28s rel_err of d_cost %.2e' % ('d_loss eps x 1.01', rel_err(E.d_loss(sc, gp, 4, 0.00101)[0], E.d_loss(sc, gp, 4, 0.001)[0])))


def trace():
    import importlib
    import pggan_amd as pg
    import test_engine_host as T
    from helpers import trace_movement_errors
    plain = E.adam
    for modname in ('engine', 'optim'):
        importlib.import_module('pggan-pytorch_amd.' + modname).ops = E
    pg.engine._check_dev = lambda t, what: t.contiguous()
    for scale in (1.0, 0.0, 1.01, 1.02):
        E.adam = (lambda *a, **k: None) if scale == 0.0 else (lambda p, g, m, v, lr, *r, **k: plain(p, g, m, v, lr * scale, *r, **k))
        losses = {}
        meta, data, G, D = T.run_trainer_trace(check_losses=False, losses_out=losses)
        E.adam = plain
        worst = max(rel_err(v, data['%s/%s' % (pre, k)]) for pre, net in (('G1', G), ('D1', D))
                    for k, v in net.reference_state_dict().items() if torch.is_tensor(v))
        dl = max(abs(a - b) / max(1.0, abs(b)) for key in 'GD' for a, b in zip(losses[key], meta[key + '_cost']))
        if scale:
            mv = trace_movement_errors(data, G=G, D=D)
            print('step x %.2f: weights rel_err %.2e, worst loss deviation %.2e, movement %.2e .. %.2e' % (scale, worst, dl, min(mv.values()), max(mv.values())))
        else:
            print('optimizer off: weights rel_err %.2e, worst loss deviation %.2e' % (worst, dl))


if __name__ == '__main__':
    {'unit': unit, 'trace': trace}[sys.argv[1] if len(sys.argv) > 1 else 'unit']()
