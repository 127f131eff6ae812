#!/usr/bin/env python
"""Device time of the k-NN-ball tile kernel (``ops.prd_kth_u8``, ``ops.prd_ball_u8``: csrc/prd.hip) against the same results composed
from the entry points that existed before it: ``ops.l2dist_u8`` in 64-row passes into a reused [64, M] int64 buffer, the diagonal
masked by index, ``ops.topk_smallest_i64`` for the radii, torch compares and sums for the counts.

    python tools/prd_time.py [--shapes 4096x1x64,4096x1x256,4096x3x256,1024x3x1024] [--k 3] [--warmup 2] [--runs 7] [--inner 1]
                             [--eval 4096x1x256,1024x3x1024] [--minibatch 16] [--json out.json]

A shape is N x C x r: two sets of N random uint8 images each, made on the device; image 1 of the second set is a copy of image 0 of
the first.  Before anything is timed both sides must agree bit for bit on the radii of both sets and on all four count vectors: the
tool stops otherwise.  Per shape ``--inner`` calls are issued between two HIP events; the figure is the median over ``--runs`` such
spans after ``--warmup`` untimed ones, divided by ``--inner``, with the minimum and the maximum as the spread; the two paths alternate
span by span.  TOP/s = 2 N^2 D / time of the fused call (its second launch included), the fraction is of the 5e15 dense int8 peak.
``--eval``: one whole ``metrics.PrecisionRecall`` evaluation without the generator passes -- ``fit()`` (the radii of the reals),
N fp32 samples fed ``--minibatch`` at a time (quantised and kept), ``result()`` (the radii of the fakes, the ball pass, one host read)
-- in wall-clock time around device synchronisations.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

INT8_PEAK = 5.0e15
I64_MAX = 0x7fffffffffffffff


def span(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    return a, b


def timed(fns, warmup, runs, inner):
    """(median, min, max) microseconds per call of every function of ``fns``, the functions alternating span by span."""
    for _ in range(warmup):
        for fn in fns:
            span(fn, inner)
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(runs):
        events = [span(fn, inner) for fn in fns]
        torch.cuda.synchronize()
        for t, (a, b) in zip(times, events):
            t.append(a.elapsed_time(b) * 1e3 / inner)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x1x64,4096x1x256,4096x3x256,1024x3x1024')
    ap.add_argument('--eval', default='4096x1x256,1024x3x1024')
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--inner', type=int, default=1)
    ap.add_argument('--minibatch', type=int, default=16)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops = pg.ops
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    k, Q = args.k, ops.NN_MAX_QUERIES
    print('%s, torch %s; k = %d, PRD_TILE = %d, passes of %d rows in the composition' % (torch.cuda.get_device_name(dev), torch.__version__, k,
                                                                                       ops.PRD_TILE, Q))
    print('%-20s %12s %14s %8s %12s %14s %8s %9s %7s' % ('sets', 'kth us', 'composed us', 'ratio', 'ball us', 'composed us', 'ratio',
                                                         'ball TOP/s', 'of peak'))
    rows = []
    g = torch.Generator(device=dev).manual_seed(1)
    for shape in [s for s in args.shapes.split(',') if s]:
        N, C, r = (int(v) for v in shape.split('x'))
        D = C * r * r
        a = torch.randint(0, 256, (N, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        b = torch.randint(0, 256, (N, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        b[1].copy_(a[0])
        buf = torch.empty((Q, N), dtype=torch.int64, device=dev)
        diag = torch.arange(Q, device=dev)

        def kth_composed(x=a):
            out = torch.empty((N,), dtype=torch.int64, device=dev)
            for i0 in range(0, N, Q):
                n = min(Q, N - i0)
                ops.l2dist_u8(x, x[i0:i0 + n], out=buf[:n])
                buf[diag[:n], i0 + diag[:n]] = I64_MAX                     # the exclusion is by index
                out[i0:i0 + n] = ops.topk_smallest_i64(buf[:n], k)[0][:, k - 1]
            return out

        rad_a, rad_b = ops.prd_kth_u8(a, k), ops.prd_kth_u8(b, k)

        def ball_composed():
            a_cnt, a_hit = (torch.empty((N,), dtype=torch.int32, device=dev) for _ in range(2))
            b_cnt, b_hit = (torch.zeros((N,), dtype=torch.int32, device=dev) for _ in range(2))
            for i0 in range(0, N, Q):
                n = min(Q, N - i0)
                ops.l2dist_u8(b, a[i0:i0 + n], out=buf[:n])
                inside_b = buf[:n] <= rad_b[None]
                inside_a = buf[:n] <= rad_a[i0:i0 + n, None]
                a_cnt[i0:i0 + n] = inside_b.sum(dim=1, dtype=torch.int32)
                a_hit[i0:i0 + n] = inside_a.sum(dim=1, dtype=torch.int32)
                b_hit += inside_b.sum(dim=0, dtype=torch.int32)
                b_cnt += inside_a.sum(dim=0, dtype=torch.int32)
            return a_cnt, a_hit, b_cnt, b_hit

        def kth_fused():
            return ops.prd_kth_u8(a, k)

        def ball_fused():
            return ops.prd_ball_u8(a, b, rad_a, rad_b)

        # exactness first
        if not (torch.equal(rad_a, kth_composed(a)) and torch.equal(rad_b, kth_composed(b))):
            raise SystemExit('%s: the radii of the two paths differ: nothing timed' % shape)
        fused, composed = ball_fused(), ball_composed()
        if not all(torch.equal(f, c) for f, c in zip(fused, composed)):
            raise SystemExit('%s: the counts of the two paths differ: nothing timed' % shape)
        if int(fused[0][0]) < 1 or int(fused[3][1]) < 1:
            raise SystemExit('%s: the planted copy is not inside its ball: nothing timed' % shape)
        kf, kc, bf, bc = timed([kth_fused, kth_composed, ball_fused, ball_composed], args.warmup, args.runs, args.inner)
        tops = 2.0 * N * N * D / bf[0] / 1e6
        rows.append({'N': N, 'C': C, 'r': r, 'D': D, 'k': k, 'kth_us': kf, 'kth_composed_us': kc, 'ball_us': bf, 'ball_composed_us': bc,
                     'kth_ratio': kc[0] / kf[0], 'ball_ratio': bc[0] / bf[0], 'ball_tops': tops, 'kth_tops': 2.0 * N * N * D / kf[0] / 1e6,
                     'int8_peak_fraction': tops * 1e12 / INT8_PEAK})
        print('%-20s %12.1f %14.1f %8.2f %12.1f %14.1f %8.2f %9.1f %6.1f%%   (spread: kth %.1f-%.1f / %.1f-%.1f, ball %.1f-%.1f / %.1f-%.1f us)'
              % ('2 x %d x %d x %d^2' % (N, C, r), kf[0], kc[0], kc[0] / kf[0], bf[0], bc[0], bc[0] / bf[0], tops, 100 * tops * 1e12 / INT8_PEAK,
                 kf[1], kf[2], kc[1], kc[2], bf[1], bf[2], bc[1], bc[2]), flush=True)
        del a, b, buf, rad_a, rad_b, fused, composed
        torch.cuda.empty_cache()
    evals = []
    for shape in [s for s in args.eval.split(',') if s]:
        N, C, r = (int(v) for v in shape.split('x'))
        stack = torch.randint(0, 256, (N, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        batch = torch.rand((args.minibatch, C, r, r), device=dev, generator=g) * 2 - 1
        metric = pg.metrics.PrecisionRecall(stack, k=k)
        best = None
        for _ in range(1 + max(1, args.runs // 3)):                          # the first round warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metric.fit()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for s in range(0, N, args.minibatch):
                metric.feed(batch[:min(args.minibatch, N - s)])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res = metric.result()
            t3 = time.perf_counter()
            best = (t1 - t0, t2 - t1, t3 - t2)
        evals.append({'N': N, 'C': C, 'r': r, 'fit_s': best[0], 'feed_s': best[1], 'result_s': best[2], 'result': res})
        print('evaluation %d reals + %d fakes of %d x %d^2: fit %.4f s, feed %.4f s (%d batches of %d), result %.4f s'
              % (N, N, C, r, best[0], best[1], -(-N // args.minibatch), args.minibatch, best[2]), flush=True)
        del stack, batch, metric
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'k': k, 'runs': args.runs, 'warmup': args.warmup, 'inner': args.inner,
                       'rows': rows, 'evaluations': evals}, f, indent=1)


if __name__ == '__main__':
    main()
