#!/usr/bin/env python
"""Device cost of the smoothed generator (ema.GeneratorEMA): the kernel alone, and the 1024x1024 train step with and without it.

    python tools/ema_time.py kernel  [--n N] [--reps 40]
    python tools/ema_time.py step    [--ema none|off|on] [--tree DIR] [--depth 8] [--minibatch 3] [--prime 50] [--steps 60] [--windows 5]
    python tools/ema_time.py compare --parent-tree DIR [--rounds 3] [step options]

``kernel``: ``pg_ema_f32`` next to ``pg_adam`` (beta1 = 0, as the trainer runs it) at the same element count -- by default the flat
parameter count of the 1024x1024 generator -- in the same run, launches alternating, each bracketed with two HIP events; median us
and GB/s (3 streams of 4 N bytes for the average, 6 for Adam: the yardstick with the same access pattern).
``step``: bench.py's method -- the Trainer loop on device-resident synthetic batches, Adam at lr 0, priming steps, then the median of
``--windows`` timed windows of ``--steps`` steps -- with ``Trainer(g_ema=GeneratorEMA(G))`` (on), ``g_ema=None`` (off), or without the
keyword (none: also runs on a tree from before the feature).  ``--tree``: the checkout whose package is measured (default: this one).
``compare``: fresh processes of ``step``, interleaved round by round: the parent checkout (none), this one with the average off and
on; prints every run, the medians and the spread of each configuration.  Stops at the first run that fails.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import(tree):
    sys.path.insert(0, os.path.abspath(tree or HERE))
    import torch
    if not torch.cuda.is_available():
        sys.exit('ema_time.py needs a GPU')
    import pggan_amd as pg
    return torch, pg


def kernel(args):
    torch, pg = _import(args.tree)
    n = args.n
    if not n:
        n = pg.Generator((1, 3, 1024, 1024))._flat_param.numel()
    gen = torch.Generator(device='cuda').manual_seed(1)
    avg, p, g = [torch.randn(n, device='cuda', generator=gen) for _ in range(3)]
    m, v = torch.zeros_like(p), torch.ones_like(p)
    ema_us, adam_us = [], []
    for i in range(args.warmup + args.reps):
        a, b, c, d = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        a.record()
        pg.ops.ema(avg, p, 0.999)
        b.record()
        c.record()
        pg.ops.adam(p, g, m, v, 0.0, 0.0, 0.99, 1e-8, 1.0, 1.0)
        d.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ema_us.append(1e3 * a.elapsed_time(b))
            adam_us.append(1e3 * c.elapsed_time(d))
    e, ad = statistics.median(ema_us), statistics.median(adam_us)
    out = {'n': n, 'reps': args.reps, 'ema_us': e, 'ema_gbs': 3 * 4 * n / e * 1e-3, 'ema_us_min_max': [min(ema_us), max(ema_us)],
           'adam_us': ad, 'adam_gbs': 6 * 4 * n / ad * 1e-3, 'adam_us_min_max': [min(adam_us), max(adam_us)]}
    print('[ema_time] n = %d (%.1f MB per stream), median of %d alternating launches' % (n, 4e-6 * n, args.reps))
    print('[ema_time] pg_ema_f32 %8.1f us  %7.0f GB/s  (3 streams; %.1f .. %.1f us)' % (e, out['ema_gbs'], min(ema_us), max(ema_us)))
    print('[ema_time] pg_adam    %8.1f us  %7.0f GB/s  (6 streams; %.1f .. %.1f us)' % (ad, out['adam_gbs'], min(adam_us), max(adam_us)))
    print(json.dumps(out))


def step(args):
    torch, pg = _import(args.tree)
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
    kw = {}
    if args.ema == 'on':
        kw['g_ema'] = pg.GeneratorEMA(G)
    elif args.ema == 'off':
        kw['g_ema'] = None
    tr = pg.Trainer(D, G, pg.wgan_gp_D_loss, pg.wgan_gp_G_loss, opt_d, opt_g, ds, ds.loader(args.minibatch),
                    pg.utils.device_latents(args.minibatch, G.latent_size, seed=1344, ring=16), **kw)
    for _ in range(args.prime):
        tr.train()
    ms = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.train()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
    out = {'tree': os.path.abspath(args.tree or HERE), 'ema': args.ema, 'depth': args.depth, 'minibatch': args.minibatch,
           'ms_per_step': statistics.median(ms), 'windows_ms': ms, 'steps_per_window': args.steps}
    print('[ema_time] step %s ema=%s: %.3f ms (windows: %s)' % (out['tree'], args.ema, out['ms_per_step'], ' '.join('%.3f' % x for x in ms)))
    print(json.dumps(out))
    return out


def compare(args):
    configs = [('parent', args.parent_tree, 'none'), ('off', None, 'off'), ('on', None, 'on')]
    runs = {name: [] for name, _, _ in configs}
    for r in range(args.rounds):
        for name, tree, ema in configs:
            cmd = [sys.executable, os.path.abspath(__file__), 'step', '--ema', ema, '--depth', str(args.depth), '--minibatch', str(args.minibatch),
                   '--prime', str(args.prime), '--steps', str(args.steps), '--windows', str(args.windows)] + (['--tree', tree] if tree else [])
            done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.run_timeout)
            if done.returncode != 0:
                sys.exit('[ema_time] %s failed with status %d: nothing more is started' % (' '.join(cmd), done.returncode))
            out = json.loads(done.stdout.strip().splitlines()[-1])
            runs[name].append(out['ms_per_step'])
            print('[ema_time] round %d %-6s %.3f ms' % (r, name, out['ms_per_step']), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    out = {'runs_ms': runs, 'median_ms': med, 'spread_ms': spread, 'off_minus_parent_ms': med['off'] - med['parent'],
           'on_minus_parent_ms': med['on'] - med['parent'], 'depth': args.depth, 'minibatch': args.minibatch}
    for k in runs:
        print('[ema_time] %-6s median %.3f ms  spread %.3f ms  (%s)' % (k, med[k], spread[k], ' '.join('%.3f' % x for x in runs[k])))
    print('[ema_time] off - parent %+.3f ms   on - parent %+.3f ms' % (out['off_minus_parent_ms'], out['on_minus_parent_ms']))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'step', 'compare'])
    ap.add_argument('--tree', default=None)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--ema', choices=['none', 'off', 'on'], default='on')
    ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--minibatch', type=int, default=3)
    ap.add_argument('--prime', type=int, default=50)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--run-timeout', type=int, default=300)
    args = ap.parse_args()
    if args.mode == 'compare' and not args.parent_tree:
        ap.error('compare needs --parent-tree')
    {'kernel': kernel, 'step': step, 'compare': compare}[args.mode](args)


if __name__ == '__main__':
    main()
