#!/usr/bin/env python
"""Time of one snapshot of generated sound, three ways, in one run (docs/experiments_magif.md):

    DeviceSoundSaver(mode='magif').to_waveforms     spectrum, pieces, overlap-add, normalise: four launches
    SoundSaver(mode='magif').image_to_sound         the same definitions in numpy on the host, sample by sample
    DeviceSoundSaver(mode='abslog').to_waveforms    Griffin-Lim with --rounds rounds (default 100): 1 + 2 x rounds launches + normalise

    python tools/magif_timing.py [--sides 256 1024] [--samples 6] [--hop 128] [--rounds 100] [--warmup 2] [--runs 7] [--inner 20]
                                 [--json out.json]

For each side, ``--samples`` seeded two-channel images in (-1, 1).  The device figures are HIP events around ``--inner`` back-to-back
calls of the magif saver, divided by ``--inner``, and around one call of the Griffin-Lim saver (the upload of its random starts
included; the copy of the waveforms back excluded from both), the host figure a wall clock around the loop over the samples; all after
``--warmup`` untimed calls, the median of ``--runs``, the three measured alternately so that they see the same machine.  The two magif
paths are compared first (1e-5 of a peak of 1, the end-to-end bound): the tool stops if they differ.  Needs a GPU; there is no
fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def device_ms(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def host_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sides', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--samples', type=int, default=6)
    ap.add_argument('--hop', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    pg.ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    print('%s, torch %s; %d samples, hop %d, Griffin-Lim rounds %d' % (torch.cuda.get_device_name(dev), torch.__version__, args.samples,
                                                                      args.hop, args.rounds))
    print('%-6s %16s %16s %18s %12s %12s' % ('side', 'magif device ms', 'magif host ms', 'abslog device ms', 'host/device', 'abslog/magif'))
    rows = []
    for side in args.sides:
        rs = np.random.RandomState(side)
        out = (rs.rand(args.samples, 2, side, side) * 2 - 1).astype(np.float32)
        out_d = torch.from_numpy(out).to(dev)
        kw = dict(create_subdirs=False, resolution=side, hop_length=args.hop, seed=1)
        magif_d, magif_h = pg.DeviceSoundSaver(mode='magif', **kw), pg.SoundSaver(mode='magif', **kw)
        abslog_d = pg.DeviceSoundSaver(mode='abslog', griffin_lim_iter=args.rounds, **kw)

        def on_device():
            return magif_d.to_waveforms(out_d)

        def on_host():
            return [magif_h.image_to_sound(img) for img in out]

        def griffin_lim():
            return abslog_d.to_waveforms(out_d[:, :1])
        diff = float(np.abs(on_device().cpu().numpy() - np.stack(on_host())).max())
        if not diff < 1e-5:
            raise SystemExit('side %d: the device and the host waveforms differ by %.3e: nothing timed' % (side, diff))
        for _ in range(args.warmup):
            on_device(), griffin_lim()
        torch.cuda.synchronize()
        t_d, t_h, t_g = [], [], []
        for _ in range(args.runs):
            t_d.append(device_ms(on_device, args.inner))
            t_h.append(host_ms(on_host))
            t_g.append(device_ms(griffin_lim))
        d, h, g = statistics.median(t_d), statistics.median(t_h), statistics.median(t_g)
        rows.append({'side': side, 'samples': args.samples, 'hop': args.hop, 'rounds': args.rounds, 'inner': args.inner, 'max_abs_diff_device_host': diff,
                     'magif_device_ms': d, 'magif_host_ms': h, 'abslog_device_ms': g, 'magif_device_ms_min_max': [min(t_d), max(t_d)],
                     'magif_host_ms_min_max': [min(t_h), max(t_h)], 'abslog_device_ms_min_max': [min(t_g), max(t_g)]})
        print('%-6d %16.3f %16.1f %18.2f %12.1f %12.1f' % (side, d, h, g, h / d, g / d))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'runs': args.runs, 'warmup': args.warmup, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
