#!/usr/bin/env python
"""Device time of one nearest-neighbour search over a uint8 image stack in HBM (``ops.nn_search_u8``: pg_l2dist_u8 on the int8 MFMA +
pg_topk_smallest_i64), against the same search composed from torch device ops: the stack converted to fp32 in chunks, one matmul per
chunk for the cross term, the norms added, ``torch.sort(stable=True)`` (inexact: fp32 sums over up to 3 M terms).

    python tools/nn_time.py [--shapes 1000x3x1024x16,1000x3x1024x64,16384x3x128x64,65536x1x32x64] [--k 3] [--warmup 2] [--runs 7]
                            [--inner 3] [--chunk-mb 512] [--json out.json]

A shape is M x C x r x K.  The stack and the queries are random bytes made on the device; queries 0 and K - 1 are copies of stack
images.  Before anything is timed the distances of the first and last 8 stack images are compared with an exact int64 evaluation in
torch and the planted copies must come back at distance 0: the tool stops otherwise.  Per shape ``--inner`` searches are issued
between two HIP events; the figure is the median over ``--runs`` such spans after ``--warmup`` untimed ones, divided by ``--inner``;
the two paths alternate span by span.  GB/s = stack bytes / time of the distance kernel (each launch of up to ops.NN_MAX_QUERIES
queries reads the stack once).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def span(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    return a, b


def timed(fns, warmup, runs, inner):
    """Median microseconds per call of every function of ``fns``, the functions alternating span by span."""
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
    ap.add_argument('--shapes', default='1000x3x1024x16,1000x3x1024x64,16384x3x128x64,65536x1x32x64')
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=512, help='fp32 bytes of one chunk of the torch composition')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops = pg.ops
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    print('%s, torch %s; k = %d, NN_MAX_QUERIES = %d' % (torch.cuda.get_device_name(dev), torch.__version__, args.k, ops.NN_MAX_QUERIES))
    print('%-22s %4s %12s %10s %10s %12s %14s %8s' % ('stack', 'K', 'search us', 'l2dist us', 'topk us', 'stack GB/s', 'torch ops us', 'ratio'))
    rows = []
    g = torch.Generator(device=dev).manual_seed(1)
    for shape in args.shapes.split(','):
        M, C, r, K = (int(v) for v in shape.split('x'))
        D = C * r * r
        stack = torch.randint(0, 256, (M, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        queries = torch.randint(0, 256, (K, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        queries[0].copy_(stack[M // 3])
        queries[K - 1].copy_(stack[M - 1])
        k = min(args.k, M)

        def search():
            return ops.nn_search_u8(stack, queries, k)

        dist = torch.empty((K, M), dtype=torch.int64, device=dev)

        def l2dist():
            return ops.l2dist_u8(stack, queries, out=dist)

        def topk():
            return ops.topk_smallest_i64(dist, k)

        step = max(1, (args.chunk_mb << 20) // (4 * D))
        qf = queries.view(K, D).float()
        qn = (qf * qf).sum(dim=1)

        def composed():
            parts = []
            for a in range(0, M, step):
                xf = stack[a:a + step].view(-1, D).float()
                parts.append(qn[:, None] - 2.0 * (qf @ xf.t()) + (xf * xf).sum(dim=1)[None])
            d = torch.cat(parts, dim=1)
            v, i = torch.sort(d, dim=1, stable=True)
            return v[:, :k], i[:, :k]

        # exactness first
        l2dist()
        some = torch.cat([torch.arange(0, min(8, M)), torch.arange(max(0, M - 8), M)]).to(dev)
        sub = stack[some].view(-1, D).long()
        exact = torch.stack([((sub - q.view(1, D).long()) ** 2).sum(dim=1) for q in queries])          # (one query at a time: memory)
        del sub
        if not torch.equal(dist[:, some], exact):
            raise SystemExit('%s: the distances differ from the exact int64 evaluation: nothing timed' % shape)
        sq, ix = search()
        if (int(sq[0, 0]), int(ix[0, 0]), int(sq[K - 1, 0]), int(ix[K - 1, 0])) != (0, M // 3, 0, M - 1):
            raise SystemExit('%s: the planted copies did not come back at distance 0: nothing timed' % shape)
        agree = float((composed()[1][:, 0] == ix[:, 0]).float().mean())
        (s_us, l_us, t_us, c_us) = timed([search, l2dist, topk, composed], args.warmup, args.runs, args.inner)
        passes = -(-K // ops.NN_MAX_QUERIES)
        gbs = passes * M * D / l_us[0] / 1e3
        rows.append({'M': M, 'C': C, 'r': r, 'K': K, 'k': k, 'stack_bytes': M * D, 'passes': passes, 'search_us': s_us, 'l2dist_us': l_us,
                     'topk_us': t_us, 'torch_ops_us': c_us, 'stack_gb_per_s': gbs, 'torch_nearest_agrees': agree})
        print('%-22s %4d %12.1f %10.1f %10.1f %12.1f %14.1f %8.2f   (torch fp32 names the same nearest image for %.0f %% of the queries)'
              % ('%d x %d x %d^2' % (M, C, r), K, s_us[0], l_us[0], t_us[0], gbs, c_us[0], c_us[0] / s_us[0], 100 * agree), flush=True)
        del stack, queries, dist, qf, qn, exact
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'k': args.k, 'runs': args.runs, 'warmup': args.warmup, 'inner': args.inner,
                       'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
