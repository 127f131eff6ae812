#!/usr/bin/env python
"""Device cost of the sound output step (sound.DeviceSoundSaver) next to the host ``SoundSaver`` on the same machine.

    python tools/griffinlim_time.py [--sizes 256 1024] [--samples 6] [--rounds 100] [--reps 7] [--warmup 2] [--host-rounds 5] [--cpus 16]

Per image size: ``DeviceSoundSaver.to_waveforms`` for ``--samples`` device samples and ``--rounds`` Griffin-Lim rounds, bracketed
with two HIP events on the current stream (the upload of the random starts included: it is part of the call); ``--warmup`` untimed
calls first, then the median of ``--reps``.  The two kernels of a round are then timed by themselves over the same buffers, ``--rounds``
launches of each between two events, which gives the per-round time of each and its share of the round.
The host yardstick is ``SoundSaver.reconstruct_from_magnitude`` on ONE sample for ``--host-rounds`` rounds (wall clock, the process
confined to ``--cpus`` CPUs), reported per round and scaled to samples x rounds -- the rounds of the host loop all do the same work.
Prints one JSON line per size.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _events(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(torch, pg, np, size, args):
    hop = 128
    gen = torch.Generator(device='cuda').manual_seed(size)
    out = torch.rand((args.samples, 1, size, size), device='cuda', generator=gen) * 2 - 1
    saver = pg.DeviceSoundSaver(create_subdirs=False, resolution=size, hop_length=hop, griffin_lim_iter=args.rounds, seed=1)
    for _ in range(args.warmup):
        saver.to_waveforms(out)
    total = [_events(torch, lambda: saver.to_waveforms(out)) for _ in range(args.reps)]
    # the two kernels of a round by themselves
    spec = pg.ops.gl_spectrum(out)
    x = torch.randn((args.samples, (size - 1) * hop), device='cuda', dtype=torch.float64, generator=gen)
    pieces = pg.ops.gl_pieces(x, spec, hop)
    y = pg.ops.overlap_add(pieces, hop)
    torch.cuda.synchronize()

    def loop(fn):
        def run():
            for _ in range(args.rounds):
                fn()
        return run
    t_pieces = [_events(torch, loop(lambda: pg.ops.gl_pieces(x, spec, hop, out=pieces))) / args.rounds for _ in range(args.reps)]
    t_ola = [_events(torch, loop(lambda: pg.ops.overlap_add(pieces, hop, out=y))) / args.rounds for _ in range(args.reps)]
    # host yardstick
    host = pg.SoundSaver(create_subdirs=False, hop_length=hop, griffin_lim_iter=args.host_rounds, seed=1)
    img = out[0, 0].cpu().numpy().astype(np.float64)
    mag = pg.utils.adjust_dynamic_range(np.vstack([img, np.zeros((1, size))]), (-1, 1), (0, 255))
    host.griffin_lim_iter = 1
    host.reconstruct_from_magnitude(mag)                                   # warm-up
    host.griffin_lim_iter = args.host_rounds
    t0 = time.perf_counter()
    host.reconstruct_from_magnitude(mag)
    host_round_ms = 1e3 * (time.perf_counter() - t0) / args.host_rounds
    med, p, o = statistics.median(total), statistics.median(t_pieces), statistics.median(t_ola)
    res = {'size': size, 'n_fft': 2 * size, 'frames': size, 'samples': args.samples, 'rounds': args.rounds, 'reps': args.reps,
           'device_snapshot_ms': med, 'device_snapshot_ms_min_max': [min(total), max(total)],
           'device_round_ms': med / args.rounds, 'pieces_ms_per_round': p, 'overlap_add_ms_per_round': o,
           'pieces_share': p / (p + o), 'overlap_add_share': o / (p + o),
           'host_ms_per_round_one_sample': host_round_ms, 'host_cpus': args.cpus, 'host_rounds_timed': args.host_rounds,
           'host_snapshot_s_scaled': 1e-3 * host_round_ms * args.rounds * args.samples}
    print('[griffinlim_time] %4d^2  device: %.2f ms per snapshot of %d x %d rounds (%.2f .. %.2f), %.1f us per round; '
          'pieces %.1f us (%.0f %%), overlap-add %.1f us (%.0f %%) per round'
          % (size, med, args.samples, args.rounds, min(total), max(total), 1e3 * med / args.rounds, 1e3 * p, 100 * res['pieces_share'],
             1e3 * o, 100 * res['overlap_add_share']))
    print('[griffinlim_time] %4d^2  host (%d CPUs): %.1f ms per round and sample -> %.1f s per snapshot (scaled from %d rounds of one sample)'
          % (size, args.cpus, host_round_ms, res['host_snapshot_s_scaled'], args.host_rounds))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--samples', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-rounds', type=int, default=5)
    ap.add_argument('--cpus', type=int, default=16)
    args = ap.parse_args()
    if hasattr(os, 'sched_setaffinity'):
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:args.cpus])
    for var in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS', 'OPENBLAS_NUM_THREADS'):
        os.environ.setdefault(var, str(args.cpus))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('griffinlim_time.py needs a GPU')
    import pggan_amd as pg
    for size in args.sizes:
        measure(torch, pg, np, size, args)


if __name__ == '__main__':
    main()
