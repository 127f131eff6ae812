"""Contract of ``pg_ema_f32`` for the CPU tier (test infrastructure, installed as ``emu_ops.ema`` by tests/test_ema_host.py) and the fp64
reference / derived bound both tiers hold ``ops.ema`` and ``GeneratorEMA`` to."""
import numpy as np
import torch

EPS = 2.0 ** -23


def omb32(beta):
    """1 - beta as the library takes it: the fp32 value ``1.f - beta``."""
    return float(np.float32(1.0) - np.float32(beta))


def ema(avg, p, beta):
    a = avg.double()
    avg.copy_((a + omb32(beta) * (p.double() - a)).float())      # (one rounding: inside the two the kernel is allowed)


def reference(avg, p, beta):
    """(fp64 evaluation of avg + (1-beta)*(p-avg), per-element bound): one rounding of the difference plus one of the fma, each 2^-24
    relative, is below 2^-23 * (|avg| + omb * |p - avg|)."""
    a, q, omb = np.asarray(avg, np.float64), np.asarray(p, np.float64), omb32(beta)
    return a + omb * (q - a), EPS * (np.abs(a) + omb * np.abs(q - a))


def recurrence(start, snapshots, betas):
    """The average over a sequence of parameter snapshots in fp64, and the largest per-step bound of each element.  The error of the
    fp32 average obeys e_k <= beta * e_(k-1) + b_k, so it stays below sum_j beta^j * max_k b_k: 5.7 x the largest step bound after eight
    steps at beta = 0.9 (10 x in the limit), which the tests round to 8 x."""
    avg = np.asarray(start, np.float64)
    worst = np.zeros_like(avg)
    if not isinstance(betas, (list, tuple)):
        betas = [betas] * len(snapshots)
    for snap, beta in zip(snapshots, betas):
        avg, b = reference(avg, snap, beta)
        worst = np.maximum(worst, b)
    return avg, worst


def flat64(net):
    if net._flat_param.is_cuda:
        torch.cuda.synchronize()
    return net._flat_param.detach().cpu().double().numpy()
