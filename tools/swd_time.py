#!/usr/bin/env python
"""Device time of one sliced-Wasserstein evaluation (metrics.SlicedWasserstein, or metrics.ChannelSlicedWasserstein with
``--channels`` 1, 2 or 4) at the paper's size, per phase.

    python tools/swd_time.py [--images 16384] [--resolution 128] [--patches 128] [--repeats 4] [--dirs 128] [--channels 3]
                             [--minibatch 64] [--warmup 1] [--runs 5] [--json out.json]
    python tools/swd_time.py --projection [--channels 4] [--images 16384] [--patches 128] [--dirs 128] [--runs 9] [--inner 4]
                             [--alt-lib LABEL=path/to/other/libpggan_hip.so ...]

Every launch of a phase (pyramid, gather, normalise, project, sort, L1) is bracketed with two HIP events; a run's phase time is the sum
over its launches, the figure printed is the median over ``--runs`` evaluations after ``--warmup`` untimed ones.  Batches are synthetic
fp32 device tensors (a ring of four), so neither a data loader nor the generator is part of the figures.  For the sort phase the
time of ``torch.sort(dim=1)`` on the same ``[dirs, images * patches]`` device tensor (standard normal values, which is what a unit
direction makes of normalised descriptors) is printed next to that of ``ops.swd_sort_rows_`` as a yardstick.
``--projection`` times the projection alone on one level's descriptors ``[images * patches, 49 C]``: ``ops.swd_project_c`` and, for
three channels, ``ops.swd_project`` beside it; every ``--alt-lib`` is another build of the library (e.g. one compiled with
``PGGAN_HIPCC_EXTRA=-DPG_SWD_LDS_STRIDE_C4=196``) whose ``pg_swd_project_c`` is called on the same buffers.  The variants ALTERNATE
inside every run (each is ``--inner`` launches between two events), so a drift of the device's clock meets all of them alike; printed
are the median over ``--runs`` and the spread (min .. max) of every variant, and the first output of every variant is compared bit for
bit with the first variant's.
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


class Phases(object):
    """The metric's phase_hook: brackets every ops call of an evaluation with two HIP events."""

    def __init__(self, phases):
        self.pairs = {p: [] for p in phases}

    def __call__(self, phase, fn, *args, **kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args, **kw)
        b.record()
        self.pairs[phase].append((a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        return {p: sum(a.elapsed_time(b) for a, b in pairs) for p, pairs in self.pairs.items()}


def evaluate(metric, batches, minibatch):
    """One evaluation through the metric's own feed_real / feed_fake / result(); returns (phase -> ms, wall ms, mean SWD)."""
    ph = Phases(metric.PHASES)
    metric.reset()
    metric.phase_hook = ph
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        for feed in (metric.feed_real, metric.feed_fake):
            for i, start in enumerate(range(0, metric.num_images, minibatch)):
                feed(batches[i % len(batches)][:min(minibatch, metric.num_images - start)])
        value = metric.result()['mean']                           # (synchronises)
    finally:
        metric.phase_hook = None
    wall = (time.perf_counter() - t0) * 1e3
    return ph.totals(), wall, value


def projection(args, pg):
    """The projection alone, variants alternating; returns the JSON record."""
    C, K, M = args.channels, args.dirs, args.images * args.patches
    W = pg.ops.SWD_PATCH * C
    gen = torch.Generator(device='cuda').manual_seed(1)
    desc = torch.randn(M, W, device='cuda', generator=gen)
    dirs = torch.randn(W, K, device='cuda', generator=gen)
    dirs = (dirs / dirs.pow(2).sum(dim=0, keepdim=True).sqrt()).contiguous()
    out = torch.empty(K, M, device='cuda')
    variants = [('swd_project_c', lambda: pg.ops.swd_project_c(desc, dirs, out=out))]
    if C == 3:
        variants.append(('swd_project', lambda: pg.ops.swd_project(desc, dirs, out=out)))
    for spec in args.alt_lib:
        label, path = spec.split('=', 1)
        fn = ctypes.CDLL(os.path.abspath(path)).pg_swd_project_c
        fn.argtypes, fn.restype = pg._lib.SWD_SIGNATURES['pg_swd_project_c'], pg._lib.I

        def call(fn=fn, label=label):
            pg._lib.check(fn(desc.data_ptr(), dirs.data_ptr(), out.data_ptr(), M, C, K, torch.cuda.current_stream().cuda_stream), label)
        variants.append((label, call))
    first = None
    for label, call in variants:                                  # warm-up of every variant, and the outputs agree
        call()
        torch.cuda.synchronize()
        if first is None:
            first = out.clone()
        elif not torch.equal(out, first):
            sys.exit('%s and %s disagree' % (label, variants[0][0]))
    times = {label: [] for label, _ in variants}
    for _ in range(args.runs):
        for label, call in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                call()
            b.record()
            torch.cuda.synchronize()
            times[label].append(a.elapsed_time(b) / args.inner)
    flop = 2.0 * M * K * (W + (W & 1))
    rec = {'mode': 'projection', 'channels': C, 'descriptors': M, 'width': W, 'directions': K, 'runs': args.runs, 'inner': args.inner,
           'variants': {label: {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t), 'runs_ms': t}
                        for label, t in times.items()}}
    print('[swd_time] projection of [%d, %d] on %d directions (%d channels), %d runs of %d launches, variants alternating'
          % (M, W, K, C, args.runs, args.inner))
    for label, _ in variants:
        v = rec['variants'][label]
        print('[swd_time] %-22s median %8.3f ms   min %8.3f   max %8.3f   (%.1f TFLOP/s at the median)'
              % (label, v['median_ms'], v['min_ms'], v['max_ms'], flop / v['median_ms'] * 1e-9))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=16384)
    ap.add_argument('--resolution', type=int, default=128)
    ap.add_argument('--patches', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=4)
    ap.add_argument('--dirs', type=int, default=128)
    ap.add_argument('--minibatch', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--channels', type=int, default=3, choices=(1, 2, 3, 4))
    ap.add_argument('--projection', action='store_true')
    ap.add_argument('--inner', type=int, default=4)
    ap.add_argument('--alt-lib', action='append', default=[], metavar='LABEL=PATH')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('swd_time.py needs a GPU')
    import pggan_amd as pg
    if args.projection:
        out = projection(args, pg)
        print(json.dumps(out))
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(out, f, indent=1)
        return
    kw = dict(patches_per_image=args.patches, dir_repeats=args.repeats, dirs_per_repeat=args.dirs, seed=0)
    if args.channels == 3:
        metric = pg.metrics.SlicedWasserstein(args.resolution, args.images, **kw)
    else:
        metric = pg.metrics.ChannelSlicedWasserstein(args.resolution, args.images, args.channels, **kw)
    gen = torch.Generator(device='cuda').manual_seed(1)
    batches = [torch.randn(args.minibatch, args.channels, args.resolution, args.resolution, device='cuda', generator=gen) for _ in range(4)]
    for _ in range(args.warmup):
        evaluate(metric, batches, args.minibatch)
    runs = [evaluate(metric, batches, args.minibatch) for _ in range(args.runs)]
    med = {p: statistics.median(r[0][p] for r in runs) for p in metric.PHASES}
    wall = statistics.median(r[1] for r in runs)
    M, K = metric.rows, metric.dirs_per_repeat
    sorts = 2 * metric.dir_repeats * len(metric.levels)

    # yardstick of the sort phase: torch.sort on a tensor of one projected set's shape
    proj = torch.randn(K, M, device='cuda', generator=gen)
    ours, theirs = [], []
    work, tmp = torch.empty_like(proj), torch.empty_like(proj)
    for i in range(args.warmup + args.runs):
        work.copy_(proj)
        a, b, c, d = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        a.record()
        pg.ops.swd_sort_rows_(work, tmp)
        b.record()
        c.record()
        ref = torch.sort(proj, dim=1)[0]
        d.record()
        torch.cuda.synchronize()
        if i == 0 and not torch.equal(work, ref):
            sys.exit('swd_sort_rows_ and torch.sort disagree')
        del ref
        if i >= args.warmup:
            ours.append(a.elapsed_time(b))
            theirs.append(c.elapsed_time(d))
    out = {'images': args.images, 'channels': args.channels, 'resolution': args.resolution, 'levels': metric.levels, 'descriptors_per_level': M, 'directions': K,
           'dir_repeats': metric.dir_repeats, 'minibatch': args.minibatch, 'runs': args.runs, 'swd_mean': runs[-1][2],
           'phase_ms': med, 'device_ms': sum(med.values()), 'wall_ms': wall, 'sorts_per_evaluation': sorts,
           'sort_one_ms': statistics.median(ours), 'torch_sort_one_ms': statistics.median(theirs),
           'wall_ms_runs': [r[1] for r in runs]}
    print('[swd_time] %d images at %dx%d, levels %s: %d descriptors x %d per level and set, %d x %d directions'
          % (args.images, args.resolution, args.resolution, metric.levels, M, metric.desc_width, metric.dir_repeats, K))
    for p in metric.PHASES:
        print('[swd_time] %-10s %10.2f ms' % (p, med[p]))
    print('[swd_time] device sum %10.2f ms   wall %10.2f ms   (median of %d runs; wall per run: %s)'
          % (out['device_ms'], wall, args.runs, ' '.join('%.0f' % r[1] for r in runs)))
    print('[swd_time] one sort of [%d, %d]: swd_sort_rows_ %.2f ms   torch.sort(dim=1) %.2f ms   ratio %.2f'
          % (K, M, out['sort_one_ms'], out['torch_sort_one_ms'], out['sort_one_ms'] / out['torch_sort_one_ms']))
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
