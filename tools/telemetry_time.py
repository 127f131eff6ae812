#!/usr/bin/env python
"""Device cost of the loss and weight statistics (telemetry.py, plugins.LossMonitor / HealthMonitor; docs/experiments_telemetry.md).

    python tools/telemetry_time.py segments [--reps 50]
    python tools/telemetry_time.py step     [--depth 8] [--minibatch 3] [--prime 50] [--steps 60] [--rounds 5]

``segments``: the two launches of ``SegmentStats.measure`` over the flat parameter buffers of the 1024x1024 generator and discriminator,
each call bracketed with two HIP events, next to the same table made from torch's device ops per parameter (``linalg.vector_norm``,
``abs().amax()``, ``isfinite``) in the same run, calls alternating; median us, and GB/s of parameter bytes for the kernels.
``step``: bench.py's method -- the Trainer loop on device-resident synthetic batches, Adam at lr 0, priming steps -- with and without
``LossMonitor`` on the SAME trainer, windows of ``--steps`` steps alternating round by round (the window with the monitor ends with its
read, like a tick); prints every window, the median and the spread (max - min) of each configuration and the difference of the medians.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import():
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('telemetry_time.py needs a GPU')
    import pggan_amd as pg
    return torch, pg


def _torch_table(torch, flat, segs):
    views = [flat[o:o + n] for _, o, n in segs]
    norms = torch.stack([torch.linalg.vector_norm(v) for v in views])
    amax = torch.stack([v.abs().amax() for v in views])
    bad = torch.stack([(~torch.isfinite(v)).sum() for v in views])
    return norms, amax, bad


def segments(args):
    torch, pg = _import()
    torch.manual_seed(1337)
    shape = (1, 3, 1024, 1024)
    out = {}
    for which, net in (('G', pg.Generator(shape).cuda()), ('D', pg.Discriminator(shape).cuda())):
        flat = net._flat_param
        segs = pg.telemetry.segments_of(net)
        seg = pg.SegmentStats.for_network(net)
        ours, theirs = [], []
        for i in range(args.warmup + args.reps):
            a, b, c, d = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            a.record()
            got = seg.measure(flat)
            b.record()
            c.record()
            ref = _torch_table(torch, flat, segs)
            d.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ours.append(1e3 * a.elapsed_time(b))
                theirs.append(1e3 * c.elapsed_time(d))
        rel = float(((got[:, 1].sqrt() - ref[0].double()).abs() / ref[0].double().clamp_min(1e-30)).max())
        same = bool(torch.equal(got[:, 2].float(), ref[1])) and bool(torch.equal(got[:, 3].long(), ref[2]))
        n = sum(s[2] for s in segs)
        o, t = statistics.median(ours), statistics.median(theirs)
        out[which] = {'parameters': n, 'segments': len(segs), 'chunks': seg.nchunks, 'measure_us': o, 'measure_us_min_max': [min(ours), max(ours)],
                      'measure_gbs': 4 * n / o * 1e-3, 'torch_us': t, 'torch_us_min_max': [min(theirs), max(theirs)], 'torch_launch_groups': 3 * len(segs),
                      'norm_rel_diff_vs_torch_fp32': rel, 'maxabs_and_counts_equal': same}
        print('[telemetry_time] %s: %d parameters in %d segments, %d chunks' % (which, n, len(segs), seg.nchunks))
        print('[telemetry_time] %s: SegmentStats.measure %8.1f us  %6.0f GB/s  (%.1f .. %.1f us)' % (which, o, out[which]['measure_gbs'], min(ours), max(ours)))
        print('[telemetry_time] %s: torch per parameter  %8.1f us  (%.1f .. %.1f us)   norms agree to %.1e, maxabs / counts equal: %s'
              % (which, t, min(theirs), max(theirs), rel, same))
    print(json.dumps(out))
    return out


def step(args):
    torch, pg = _import()
    torch.manual_seed(1337)
    res = 4 * 2 ** args.depth
    shape = (1, 3, 1024, 1024)
    G, D = pg.Generator(shape).cuda(), pg.Discriminator(shape).cuda()
    G.depth = D.depth = args.depth
    opt_g = pg.FusedAdam(G.parameters(), 0.0, betas=(0.0, 0.99))          # lr 0: every step runs on the seeded weights
    opt_d = pg.FusedAdam(D.parameters(), 0.0, betas=(0.0, 0.99))
    ds = pg.utils.SyntheticDataset(res, 3, seed=1337, ring=8)
    ds.model_depth = args.depth
    pg.wgan_gp_loss.manual_seed(1337)
    tr = pg.Trainer(D, G, pg.wgan_gp_D_loss, pg.wgan_gp_G_loss, opt_d, opt_g, ds, ds.loader(args.minibatch),
                    pg.utils.device_latents(args.minibatch, G.latent_size, seed=1344, ring=16))
    mon = pg.LossMonitor()
    mon.register(tr)

    def window(on):
        tr.plugin_queues['iteration'] = [(0, 0, mon)] if on else []      # the same trainer, with and without the plugin in its queue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.train()
        if on:
            mon.epoch(1)                                                 # the tick's read
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps
    for _ in range(args.prime):
        tr.train()
    window(True)
    window(False)
    runs = {'on': [], 'off': []}
    for r in range(args.rounds):
        for name in (('on', 'off') if r % 2 == 0 else ('off', 'on')):
            runs[name].append(window(name == 'on'))
            print('[telemetry_time] round %d %-3s %.3f ms' % (r, name, runs[name][-1]), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    out = {'depth': args.depth, 'minibatch': args.minibatch, 'steps_per_window': args.steps, 'windows_ms': runs, 'median_ms': med,
           'spread_ms': spread, 'on_minus_off_ms': med['on'] - med['off'], 'last_tick': {k: tr.stats[k]['val'] for k in mon.names}}
    for k in ('off', 'on'):
        print('[telemetry_time] depth %d mb %d  LossMonitor %-3s median %.3f ms  spread %.3f ms' % (args.depth, args.minibatch, k, med[k], spread[k]))
    print('[telemetry_time] on - off %+.4f ms' % out['on_minus_off_ms'])
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['segments', 'step'])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--minibatch', type=int, default=3)
    ap.add_argument('--prime', type=int, default=50)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    {'segments': segments, 'step': step}[args.mode](args)


if __name__ == '__main__':
    main()
