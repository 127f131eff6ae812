#!/usr/bin/env python
"""Device time of the k-means update pass over a uint8 image stack in HBM (``pg_cluster_sums_u8``), next to the stack-read rate of
``pg_l2dist_u8`` on the same stack in the same run, against the same update composed from torch device ops (``index_add_`` over chunks
of the stack converted to int32); then a whole ``metrics.NDB`` fit and one evaluation of ``--samples`` images fed as uint8 levels
(``--generator R`` also times the generator passes of an evaluation at R x R).

    python tools/ndb_time.py [--shapes 30000x1x64x50,4096x3x256x50,1000x3x1024x50] [--samples 8192] [--minibatch 16] [--warmup 2]
                             [--runs 7] [--inner 3] [--chunk-mb 512] [--generator 1024] [--json out.json]

A shape is M x C x r x K.  The stack is random bytes made on the device, the labels are random in 0 .. K-1 with a fifth of the images
held out (-1).  Before anything is timed the sums are compared with the torch composition (``torch.equal``): the tool stops otherwise.
Per shape ``--inner`` calls are issued between two HIP events; the figure is the median over ``--runs`` such spans after ``--warmup``
untimed ones, divided by ``--inner``; the paths alternate span by span.  The kernel is timed through the C entry on a member list
made once (the sort and the bincount of the wrapper are timed with ``cluster_sums_u8`` as a whole).  GB/s = bytes of the MEMBER
images / kernel time for the sums, stack bytes / time for the distances.  Peak memory: ``torch.cuda.max_memory_allocated`` above the
stack, per path.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

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


def peak_above(fn, base):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='30000x1x64x50,4096x3x256x50,1000x3x1024x50')
    ap.add_argument('--samples', type=int, default=8192)
    ap.add_argument('--minibatch', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=512, help='int32 bytes of one chunk of the torch composition')
    ap.add_argument('--generator', type=int, default=0, metavar='R', help='also time G.forward of the default R x R network at its last '
                    'stage, --minibatch latents per call: the other part of an NDBMonitor evaluation (0: skip)')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops, cluster, _lib = pg.ops, pg.cluster, pg._lib
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    print('%s, torch %s; samples = %d in batches of %d' % (torch.cuda.get_device_name(dev), torch.__version__, args.samples, args.minibatch))
    print('%-22s %3s %9s %9s %10s %9s %10s %6s %11s %7s %9s %9s %9s %5s %9s'
          % ('stack', 'K', 'sums us', 'GB/s', 'l2dist us', 'GB/s', 'wrapper us', 'ratio', 'torch us', 'x', 'peak MB', 'torch MB', 'fit ms', 'iter', 'eval ms'))
    rows = []
    g = torch.Generator(device=dev).manual_seed(1)
    for shape in args.shapes.split(','):
        M, C, r, K = (int(v) for v in shape.split('x'))
        D = C * r * r
        stack = torch.randint(0, 256, (M, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        label = torch.randint(0, K, (M,), device=dev, generator=g).to(torch.int32)
        label[torch.rand(M, device=dev, generator=g) < 0.2] = -1
        members = int((label >= 0).sum())
        cents = stack[:K].clone()
        key = label.to(torch.int64) + 1
        order = torch.sort(key, stable=True)[1].to(torch.int32)
        offsets = torch.cumsum(torch.bincount(key, minlength=K + 1), 0).to(torch.int32)
        sums = torch.empty((K, C, r, r), dtype=torch.int32, device=dev)
        dist = torch.empty((K, M), dtype=torch.int64, device=dev)

        def kernel():
            _lib.call('pg_cluster_sums_u8', stack.data_ptr(), M, D, order.data_ptr(), M, offsets.data_ptr(), K, sums.data_ptr(), ops._stream())

        def l2dist():
            ops.l2dist_u8(stack, cents, out=dist)

        def wrapper():
            return cluster.cluster_sums_u8(stack, label, K)

        step = max(1, (args.chunk_mb << 20) // (4 * D))
        safe = label.to(torch.int64).clamp(min=0)
        weight = (label >= 0).to(torch.int32)

        def composed():
            out = torch.zeros((K, D), dtype=torch.int32, device=dev)
            for a in range(0, M, step):
                out.index_add_(0, safe[a:a + step], stack[a:a + step].view(-1, D).to(torch.int32) * weight[a:a + step, None])
            return out

        kernel()
        if not torch.equal(sums.view(K, D), composed()) or not torch.equal(wrapper()[0], sums):
            raise SystemExit('%s: the sums differ from the torch composition: nothing timed' % shape)
        base = torch.cuda.memory_allocated()
        peak_w, peak_c = peak_above(wrapper, base), peak_above(composed, base)
        k_us, l_us, w_us, c_us = timed([kernel, l2dist, wrapper, composed], args.warmup, args.runs, args.inner)
        del sums, dist, order, offsets, safe, weight, key
        # a whole fit (host reads included: wall clock around a synchronise) and one evaluation fed as uint8 levels
        h = min(M // 5, args.samples)
        ndb = pg.metrics.NDB(stack, k=K, holdout=h)
        ndb.fit()                                                # untimed: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ndb.fit()
        torch.cuda.synchronize()
        fit_ms = (time.perf_counter() - t0) * 1e3
        fake = torch.randint(0, 256, (args.minibatch, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        evals = []
        for _ in range(3):
            ndb.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for a in range(0, args.samples, args.minibatch):
                ndb.feed_u8(fake[:min(args.minibatch, args.samples - a)])
            ndb.result()
            evals.append((time.perf_counter() - t0) * 1e3)
        eval_ms = statistics.median(evals)
        gbs_k, gbs_l = members * D / k_us[0] / 1e3, M * D / l_us[0] / 1e3
        rows.append({'M': M, 'C': C, 'r': r, 'K': K, 'stack_bytes': M * D, 'member_bytes': members * D, 'sums_us': k_us, 'l2dist_us': l_us,
                     'wrapper_us': w_us, 'torch_ops_us': c_us, 'sums_gb_per_s': gbs_k, 'l2dist_gb_per_s': gbs_l,
                     'peak_bytes_wrapper': peak_w, 'peak_bytes_torch': peak_c, 'fit_ms': fit_ms, 'iterations': ndb.iterations,
                     'converged': ndb.converged, 'eval_ms': eval_ms, 'samples': args.samples, 'minibatch': args.minibatch})
        print('%-22s %3d %9.1f %9.1f %10.1f %9.1f %10.1f %6.2f %11.1f %7.1f %9.1f %9.1f %9.1f %5d %9.1f'
              % ('%d x %d x %d^2' % (M, C, r), K, k_us[0], gbs_k, l_us[0], gbs_l, w_us[0], gbs_k / gbs_l, c_us[0], c_us[0] / w_us[0],
                 peak_w / 1e6, peak_c / 1e6, fit_ms, ndb.iterations, eval_ms), flush=True)
        del stack, label, cents, ndb, fake
        torch.cuda.empty_cache()
    generator = None
    if args.generator:
        R = args.generator
        torch.manual_seed(1)
        G = pg.Generator((1, 3, R, R)).to(dev)
        G.depth = R.bit_length() - 3                             # 4 * 2^depth = R
        z = torch.randn(args.minibatch, 512, device=dev)
        for _ in range(2):
            G.forward(z)
        torch.cuda.synchronize()
        calls = 8
        t0 = time.perf_counter()
        for _ in range(calls):
            G.forward(z)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / calls
        generator = {'resolution': R, 'minibatch': args.minibatch, 'forward_ms': ms, 'calls': calls,
                     'evaluation_s': ms * 1e-3 * -(-args.samples // args.minibatch)}
        print('G.forward at %d x %d, %d latents per call: %.2f ms per call (%d calls, wall clock around a synchronise); %d samples: %.2f s'
              % (R, R, args.minibatch, ms, calls, args.samples, generator['evaluation_s']), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'generator': generator, 'device': torch.cuda.get_device_name(dev), 'runs': args.runs, 'warmup': args.warmup, 'inner': args.inner,
                       'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
