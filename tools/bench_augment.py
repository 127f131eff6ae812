#!/usr/bin/env python
"""Device time of the differentiable augmentation (augment.py, csrc/augment.hip): the gather and its transpose alone against the copy
launch they replace, and a whole Trainer iteration with and without an Augmenter.

    python tools/bench_augment.py [--shapes 3x3x1024 16x2x256] [--stage 1024x3 256x16] [--rounds 3] [--out FILE.json] [--markdown FILE.md]

Kernels   per shape ``N x C x r`` (images [N,C,r,r]), in one process, round by round and interleaved: ``ops.axpby_mask(x, a=1.0, out=y)`` (the
          copy launch of the real third, which the augmented step replaces with ``apply``), ``apply`` and ``adjoint`` under an identity table,
          a misaligned shift (dx = 5, dy = 3), a flipped misaligned shift, and flip + shift + cutout + gain on every image.  ``--reps``
          launches of a case are captured into ONE hipGraph and the graph is replayed between two HIP events (after ``--warm`` eager
          launches and one un-timed replay), ``--windows`` replays per round: issued one by one from Python a 3 us launch is host-bound
          (the copy at 16 x 2 x 256^2 reads 4 - 6 us that way), a replayed graph is not.  Per case: the median over
          rounds x windows of the time per launch, the spread (max - min) and the bytes moved (read + written, counted from the shape: 8
          bytes per element) over the median.  ``--eager`` times the host-issued launches instead (the host cost of a wrapper).
          Target: apply and adjoint <= 2 x the copy's time (a misaligned 16-byte read touches at most two aligned words).
Iteration ``Trainer.train()`` of ``gan_losses('logistic', penalty='r1')`` with and without ``Augmenter(p=1)`` (both pairs are closures of
          gan_losses, so neither side runs the early generator pass), on device-resident synthetic batches with Adam at lr 0, the two cases
          alternating round by round on the same network pair; recorded, not gated.

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _summary(v):
    return {'median_ms': statistics.median(v), 'spread_ms': max(v) - min(v), 'windows_ms': v}


def _tables(torch, N, r):
    """name -> int32 table [N, 8]"""
    import numpy as np
    gain = int(np.float32(0.25).view(np.int32))
    rows = {'identity': [0, 0, 0, 0, 0, 0, 0, 0], 'shift dx=5 dy=3': [0, 3, 5, 0, 0, 0, 0, 0], 'flip, shift dx=5 dy=3': [1, 3, 5, 0, 0, 0, 0, 0],
            'flip, shift, cutout, gain': [3, -3, -7, r // 4, r // 2, r // 8, r // 2, gain]}
    return {k: torch.tensor([v] * N, dtype=torch.int32, device='cuda') for k, v in rows.items()}


def kernels(torch, pg, N, C, r, args):
    gen = torch.Generator(device='cuda').manual_seed(5)
    x = torch.randn((N, C, r, r), device='cuda', generator=gen)
    y = torch.empty_like(x)
    tables = _tables(torch, N, r)
    cases = [('copy (axpby_mask)', lambda: pg.ops.axpby_mask(x, a=1.0, out=y))]
    for name, t in tables.items():
        cases.append(('apply: ' + name, lambda t=t: pg.ops.augment_apply(x, t, 1, out=y)))
    for name, t in tables.items():
        cases.append(('adjoint: ' + name, lambda t=t: pg.ops.augment_adjoint(x, t, out=y)))
    times = {name: [] for name, _ in cases}
    graphs = {}
    for name, fn in cases:
        for _ in range(args.warm):
            fn()
        if not args.eager:
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(args.reps):
                    fn()
            graphs[name].replay()
    for _ in range(args.rounds):
        for name, fn in cases:
            if args.eager:
                times[name] += [_window(torch, fn, args.reps) for _ in range(args.windows)]
            else:
                times[name] += [_window(torch, graphs[name].replay, 1) / args.reps for _ in range(args.windows)]
    nbytes = 8.0 * x.numel()
    out = {'shape': [N, C, r, r], 'bytes': nbytes, 'cases': {name: _summary(v) for name, v in times.items()}}
    base = out['cases']['copy (axpby_mask)']['median_ms']
    for name, _ in cases:
        c = out['cases'][name]
        c['x_copy'] = c['median_ms'] / base
        c['gbytes_per_s'] = nbytes / c['median_ms'] / 1e6
        print('[bench_augment] %dx%dx%d^2  %-36s %8.2f us (spread %.2f)  %7.0f GB/s  x%.2f of the copy' % (
            N, C, r, name, 1e3 * c['median_ms'], 1e3 * c['spread_ms'], c['gbytes_per_s'], c['x_copy']), flush=True)
    return out


def iteration(torch, pg, res, mb, args):
    depth = {4 * 2 ** d: d for d in range(9)}[res]
    torch.manual_seed(1337)
    shape = (1, 3, 1024, 1024)
    G, D = pg.Generator(shape).cuda(), pg.Discriminator(shape).cuda()
    G.depth = D.depth = depth
    ds = pg.utils.SyntheticDataset(res, 3, seed=1337, ring=8)
    ds.model_depth = depth
    aug = pg.Augmenter(p=1.0, translate=(0.0, 0.125), cutout=(1.0, 0.125), gain=0.2, flip=False, seed=3)
    pairs = [('no augmenter', pg.gan_losses('logistic', penalty='r1')), ('Augmenter(p=1)', pg.gan_losses('logistic', penalty='r1', augment=aug))]
    times = {name: [] for name, _ in pairs}
    for rnd in range(args.rounds):
        for name, (D_loss, G_loss) in pairs:
            opt_g = pg.FusedAdam(G.parameters(), 0.0, betas=(0.0, 0.99))          # lr 0: every step runs on the seeded weights
            opt_d = pg.FusedAdam(D.parameters(), 0.0, betas=(0.0, 0.99))
            tr = pg.Trainer(D, G, D_loss, G_loss, opt_d, opt_g, ds, ds.loader(mb), pg.utils.device_latents(mb, G.latent_size, seed=1344, ring=16))
            for _ in range(args.prime):
                tr.train()
            times[name] += [_window(torch, tr.train, args.steps) for _ in range(args.windows)]
            print('[bench_augment] %dx%d round %d %-16s %.3f ms per iteration' % (res, mb, rnd, name, statistics.median(times[name][-args.windows:])), flush=True)
    out = {'resolution': res, 'minibatch': mb, 'cases': {name: _summary(v) for name, v in times.items()}}
    out['difference_ms'] = out['cases']['Augmenter(p=1)']['median_ms'] - out['cases']['no augmenter']['median_ms']
    print('[bench_augment] %dx%d  difference %.3f ms per iteration' % (res, mb, out['difference_ms']))
    pg.wgan_gp_loss.enable_graphs(False)            # drop the plans (and the activations they pin) before the next stage
    pg.wgan_gp_loss.enable_graphs('auto')
    return out


def markdown(results):
    lines = []
    for k in results['kernels']:
        N, C, r, _ = k['shape']
        lines += ['', '`%d x %d x %d^2` (%.1f MB read + %.1f MB written per launch):' % (N, C, r, k['bytes'] / 2e6, k['bytes'] / 2e6), '',
                  '| launch | us (median) | spread us | GB/s | x the copy |', '|---|---|---|---|---|']
        for name, c in k['cases'].items():
            lines.append('| %s | %.2f | %.2f | %.0f | %.2f |' % (name, 1e3 * c['median_ms'], 1e3 * c['spread_ms'], c['gbytes_per_s'], c['x_copy']))
    lines += ['', '| stage | no augmenter ms (spread) | Augmenter(p=1) ms (spread) | difference ms |', '|---|---|---|---|']
    for s in results['iterations']:
        a, b = s['cases']['no augmenter'], s['cases']['Augmenter(p=1)']
        lines.append('| %d^2, minibatch %d | %.3f (%.3f) | %.3f (%.3f) | %+.3f |' % (s['resolution'], s['minibatch'], a['median_ms'], a['spread_ms'],
                                                                                    b['median_ms'], b['spread_ms'], s['difference_ms']))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='*', default=['3x3x1024', '16x2x256'])
    ap.add_argument('--stage', nargs='*', default=['1024x3', '256x16'])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--eager', action='store_true', help='kernels: time host-issued launches instead of a replayed hipGraph')
    ap.add_argument('--prime', type=int, default=12)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--out', default=None, help='write the JSON of every measurement to this file')
    ap.add_argument('--markdown', default=None, help='write the tables of docs/experiments_augment.md to this file')
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_augment.py needs a GPU')
    import pggan_amd as pg
    results = {'kernels': [], 'iterations': []}
    for s in args.shapes:
        N, C, r = (int(v) for v in s.split('x'))
        results['kernels'].append(kernels(torch, pg, N, C, r, args))
    for s in args.stage:
        res, mb = (int(v) for v in s.split('x'))
        results['iterations'].append(iteration(torch, pg, res, mb, args))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)
    if args.markdown:
        with open(args.markdown, 'w') as f:
            f.write(markdown(results))
    print(markdown(results))


if __name__ == '__main__':
    main()
