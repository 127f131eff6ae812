#!/usr/bin/env python
"""Device time of one MS-SSIM evaluation of a batch of pairs (ops.msssim_pairs), per scale, against the same evaluation composed from
torch's device ops on the same tensors.

    python tools/msssim_time.py [--resolution 1024] [--channels 3] [--pairs 16] [--warmup 2] [--runs 5] [--bound 1e-4] [--json out.json]

Every launch (one per scale plus the final one) is bracketed with two HIP events; the figure printed is the median over ``--runs``
evaluations after ``--warmup`` untimed ones.  Next to each scale: the bytes the fused launch has to move, counted from the shapes (two
images read, two quarter-size images and the partial sums written), and that over the time.  The yardstick is the definition
composed from torch's device ops -- quantisation by elementwise ops, the five moment planes by a row and a column pass of grouped
``conv2d``, ``avg_pool2d`` between scales -- timed the same way as one span.  The two results are compared first: the tool stops if
they disagree by more than ``--bound`` (1e-4, the cap of the bound of tests/test_msssim_gpu.py: the composition is fp32 in the naive form
and is itself up to 6e-5 from the fp64 reference on flat images).  Inputs are smooth-plus-noise images generated from a
seed.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def make_inputs(n, C, R, device):
    g = torch.Generator(device=device).manual_seed(R + C)

    def smooth():
        low = torch.rand(n, C, max(R // 8, 2), max(R // 8, 2), generator=g, device=device)
        up = F.interpolate(low, size=(R, R), mode='bilinear', align_corners=False)
        return 0.3 + 0.3 * (0.75 * up + 0.25 * torch.rand(n, C, R, R, generator=g, device=device))
    a = smooth()
    return a.contiguous(), (0.5 * a + 0.5 * smooth()).contiguous()


def torch_msssim(a, b, weights, taps, drange=(-1, 1)):
    """The definition from torch's device ops, fp32.  Returns per-pair values (fp64 from the fp32 per-scale means)."""
    lo, hi = drange
    scale = torch.tensor(255.0 / (hi - lo), dtype=torch.float32, device=a.device)
    a, b = (((t - lo) * scale).round().clamp(0, 255) for t in (a, b))
    n, C = a.shape[:2]
    row = taps.view(1, 1, 1, -1).repeat(5 * C, 1, 1, 1)
    col = taps.view(1, 1, -1, 1).repeat(5 * C, 1, 1, 1)
    terms = []
    for s in range(len(weights)):
        m = F.conv2d(F.conv2d(torch.cat([a, b, a * a, b * b, a * b], dim=1), row, groups=5 * C), col, groups=5 * C)
        mu_a, mu_b, e_aa, e_bb, e_ab = m.split(C, dim=1)
        cs = (2 * (e_ab - mu_a * mu_b) + C2) / ((e_aa - mu_a * mu_a) + (e_bb - mu_b * mu_b) + C2)
        if s == len(weights) - 1:
            terms.append(((2 * mu_a * mu_b + C1) / (mu_a * mu_a + mu_b * mu_b + C1) * cs).mean(dim=(1, 2, 3)))
        else:
            terms.append(cs.mean(dim=(1, 2, 3)))
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    value = torch.ones(n, dtype=torch.float64, device=a.device)
    for t, w in zip(terms, weights):
        value = value * t.double().clamp(min=0) ** w
    return value


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return out, (a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--bound', type=float, default=1e-4)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops = pg.ops
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    n, C, R = args.pairs, args.channels, args.resolution
    sides, weights = ops.msssim_scales(R)
    a, b = make_inputs(n, C, R, dev)
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    taps = (g / g.sum()).float().to(dev)
    scratch = ops.MSSSIMScratch(n, C, R, dev)
    values = torch.empty(n, device=dev, dtype=torch.float64)
    terms = torch.empty((n, len(sides)), device=dev, dtype=torch.float64)
    partials = scratch.partials(n)

    def fused():
        """ops.msssim_pairs launch by launch, each bracketed."""
        events = []
        cur = (a, b)
        for s in range(len(sides)):
            nxt = (None, None) if s == len(sides) - 1 else scratch.pooled[s]
            _, ev = timed(lambda: ops.msssim_scale(cur[0], cur[1], nxt[0], nxt[1], partials[s], 'quantize' if s == 0 else 'as_is'))
            events.append(ev)
            cur = nxt
        _, ev = timed(lambda: pg._lib.call('pg_msssim_finish', partials[0].data_ptr(), values.data_ptr(), terms.data_ptr(), n, C, R,
                                           ops._stream()))
        events.append(ev)
        return events

    # the two must agree before either is timed
    fused()
    direct, _ = ops.msssim_pairs(a, b, scratch=scratch)
    assert torch.equal(direct, values), 'the launch-by-launch form is not ops.msssim_pairs'
    composed = torch_msssim(a, b, weights, taps)
    diff = float((values - composed).abs().max())
    print('fused vs torch composition: max abs difference of the per-pair values %.3e (bound %.1e); mean value %.4f'
          % (diff, args.bound, float(values.mean())))
    if not diff <= args.bound:
        raise SystemExit('the fused path and the torch composition disagree beyond the bound: nothing timed')

    for _ in range(args.warmup):
        fused()
        torch_msssim(a, b, weights, taps)
    torch.cuda.synchronize()
    per_launch, whole, torch_ms = [], [], []
    for _ in range(args.runs):                                               # alternating, so that both see the same machine
        (events, span) = timed(fused)
        _, tspan = timed(lambda: torch_msssim(a, b, weights, taps))
        torch.cuda.synchronize()
        per_launch.append([x.elapsed_time(y) for x, y in events])
        whole.append(span[0].elapsed_time(span[1]))
        torch_ms.append(tspan[0].elapsed_time(tspan[1]))
    med = [statistics.median(col) for col in zip(*per_launch)]
    rows = []
    print('%d pairs x %d x %dx%d, median of %d after %d warm-up' % (n, C, R, R, args.runs, args.warmup))
    print('%-10s %10s %12s %10s' % ('launch', 'ms', 'MB moved', 'GB/s'))
    for s, side in enumerate(sides):
        moved = 2 * n * C * side * side * 4 + (2 * n * C * (side // 2) ** 2 * 4 if s < len(sides) - 1 else 0) + partials[s].numel() * 8
        rows.append({'launch': 'scale %d' % side, 'ms': med[s], 'bytes': moved, 'gb_per_s': moved / med[s] / 1e6})
        print('%-10s %10.4f %12.2f %10.1f' % ('scale %d' % side, med[s], moved / 1e6, moved / med[s] / 1e6))
    rows.append({'launch': 'finish', 'ms': med[-1]})
    print('%-10s %10.4f' % ('finish', med[-1]))
    fused_ms, comp_ms = statistics.median(whole), statistics.median(torch_ms)
    print('fused, whole span       %10.4f ms   (min %.4f, max %.4f)' % (fused_ms, min(whole), max(whole)))
    print('torch composition       %10.4f ms   (min %.4f, max %.4f)' % (comp_ms, min(torch_ms), max(torch_ms)))
    print('ratio torch / fused     %10.2f' % (comp_ms / fused_ms))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'pairs': n, 'channels': C, 'resolution': R, 'rows': rows, 'fused_ms': fused_ms, 'torch_ms': comp_ms,
                       'ratio': comp_ms / fused_ms, 'max_abs_difference': diff, 'runs': args.runs, 'warmup': args.warmup}, f, indent=1)


if __name__ == '__main__':
    main()
