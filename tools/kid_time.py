#!/usr/bin/env python
"""Device time of the tile sums of the kernel distance (``ops.kid_tilesums_f64``: csrc/kid.hip) against the same sums composed from
torch's device ops, beside ``ops.fd_moments_f64`` on the same features, and the host-visible cost of one ``KernelDistance.result()``.

    python tools/kid_time.py [--shapes 4096x4096x128,30000x4096x128,30000x0x128] [--moments 30000x128] [--result 30000x4096x128]
                             [--warmup 1] [--runs 5] [--no-composed] [--json out.json]

A shape is M x N x F: random float32 features made on the device; N = 0 is the self form with ``skip_diagonal``.  Per shape, between
two HIP events, the median over ``--runs`` spans after ``--warmup`` untimed ones, with the minimum and the maximum as the spread, the
paths alternating:
  fused     ``ops.kid_tilesums_f64`` (the output allocated once, outside the span)
  composed  ``((gamma * x.double() @ y.double().T + coef0) ** 3).sum()`` in row chunks whose fp64 Gram block is at most 1 GiB -- one
            number per chunk, where the fused path leaves one per tile; the self form subtracts the diagonal's kernel values.  The
            tool stops if the two totals differ by more than 1e-9 of the total.
The rate is 2 F x (pairs of the tiles computed) / time: all A B tiles of the cross form, the A (A + 1) / 2 tiles on or above the
diagonal of the self form.  ``--moments`` M x F: ``ops.fd_moments_f64`` on the same kind of features, with its rate by 2 M F^2, for
comparison.  ``--result`` M x N x F: what ``metrics.KernelDistance`` adds to an evaluation, in wall-clock time around device
synchronisations: the reals' self sums (``fit()``, once per stage), and the fakes' self sums, the cross sums, the host read and
``metrics.kid_statistic`` (``result()``).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def span(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def timed(fns, warmup, runs):
    """(median, min, max) milliseconds per call of every function of ``fns``, the functions alternating span by span."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(runs):
        events = [span(fn) for fn in fns]
        torch.cuda.synchronize()
        for t, (a, b) in zip(times, events):
            t.append(a.elapsed_time(b))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def composed_total(x, y, gamma, coef0):
    """The sum over all pairs (the self form: without i == j) from torch's device ops, as a device scalar."""
    other = x if y is None else y
    yd = other.double().t().contiguous()
    rows = max(1, (1 << 30) // (8 * other.shape[0]))
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for s in range(0, x.shape[0], rows):
        total += ((gamma * (x[s:s + rows].double() @ yd) + coef0) ** 3).sum()
    if y is None:
        total -= ((gamma * x.double().pow(2).sum(dim=1) + coef0) ** 3).sum()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x4096x128,30000x4096x128,30000x0x128')
    ap.add_argument('--moments', default='30000x128')
    ap.add_argument('--result', default='30000x4096x128')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-composed', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops, metrics = pg.ops, pg.metrics
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    T = ops.KID_TILE
    print('%s, torch %s; KID_TILE = %d' % (torch.cuda.get_device_name(dev), torch.__version__, T))
    g = torch.Generator(device=dev).manual_seed(1)
    feats = lambda rows, F: (0.4 * torch.randn((rows, F), device=dev, generator=g) + 0.3).contiguous()
    rows, moments, results = [], [], []
    for shape in [s for s in args.shapes.split(',') if s]:
        M, N, F = (int(v) for v in shape.split('x'))
        x, y = feats(M, F), feats(N, F) if N else None
        gamma, coef0 = 1.0 / F, 1.0
        A, B = (M + T - 1) // T, ((N or M) + T - 1) // T
        out = torch.empty((A, B), dtype=torch.float64, device=dev)
        fns = [lambda: ops.kid_tilesums_f64(x, y, gamma, coef0, skip_diagonal=not N, out=out)]
        row = {'M': M, 'N': N, 'F': F}
        if not args.no_composed:
            a, b = float(fns[0]().sum()), float(composed_total(x, y, gamma, coef0))
            if not abs(a - b) <= 1e-9 * abs(b):
                raise SystemExit('%s: the totals of the two paths differ, %.15g against %.15g: nothing timed' % (shape, a, b))
            row['total_difference'] = abs(a - b) / abs(b)
            fns.append(lambda: composed_total(x, y, gamma, coef0))
        res = timed(fns, max(1, args.warmup), args.runs)
        tiles = A * B if N else A * (A + 1) // 2
        rate = 2.0 * F * tiles * T * T / (res[0][0] * 1e-3)
        row.update(fused_ms=res[0], flops_per_s=rate, tiles=tiles)
        text = ''
        if not args.no_composed:
            row['composed_ms'] = res[1]
            text = '; composed from torch ops %.3f ms (%.3f-%.3f), ratio %.2f, totals differ by %.1e of the total' \
                   % (res[1][0], res[1][1], res[1][2], res[1][0] / res[0][0], row['total_difference'])
        rows.append(row)
        print('tile sums %6d x %6d x %3d%s: %.4f ms (%.4f-%.4f), %d tiles, %.3f Tflop/s fp64%s'
              % (M, N or M, F, '' if N else ' (self)', res[0][0], res[0][1], res[0][2], tiles, rate / 1e12, text), flush=True)
        del x, y, out
        torch.cuda.empty_cache()
    for shape in [s for s in args.moments.split(',') if s]:
        M, F = (int(v) for v in shape.split('x'))
        x = feats(M, F)
        (t,) = timed([lambda: ops.fd_moments_f64(x)], max(1, args.warmup), args.runs)
        rate = 2.0 * M * F * F / (t[0] * 1e-3)
        moments.append({'M': M, 'F': F, 'ms': t, 'flops_per_s': rate})
        print('moments   %6d x %3d: %.4f ms (%.4f-%.4f), %.3f Tflop/s fp64 by 2 M F^2' % (M, F, t[0], t[1], t[2], rate / 1e12), flush=True)
    for shape in [s for s in args.result.split(',') if s]:
        M, N, F = (int(v) for v in shape.split('x'))
        x, y = feats(M, F), feats(N, F)
        best = None
        for _ in range(2):                                                   # the first round warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sxx = ops.kid_tilesums_f64(x, skip_diagonal=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            syy, sxy = ops.kid_tilesums_f64(y, skip_diagonal=True), ops.kid_tilesums_f64(x, y)
            host = torch.cat([sxx.reshape(-1), syy.reshape(-1), sxy.reshape(-1)]).cpu().numpy()
            a, b = sxx.numel(), sxx.numel() + syy.numel()
            res = metrics.kid_statistic(host[:a].reshape(sxx.shape), host[a:b].reshape(syy.shape), host[b:].reshape(sxy.shape), M, N)
            t2 = time.perf_counter()
            best = (t1 - t0, t2 - t1)
        results.append({'M': M, 'N': N, 'F': F, 'fit_sums_s': best[0], 'result_s': best[1], 'kid': res['kid'], 'subsets': res['subsets'],
                        'kid_subset_std': res['kid_subset_std']})
        print('evaluation %d reals, %d samples, %d features: the reals\' sums (once per stage) %.4f s; result() -- two launches, the host '
              'read, the statistic over %d subsets -- %.4f s; kid %.3e (std over subsets %.3e)'
              % (M, N, F, best[0], res['subsets'], best[1], res['kid'], res['kid_subset_std'] or float('nan')), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'runs': args.runs, 'warmup': args.warmup, 'tile_sums': rows,
                       'moments': moments, 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
