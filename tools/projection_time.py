#!/usr/bin/env python
"""Device time of the latent projection (docs/experiments_projection.md): the pyramid-loss kernel alone, one projection step per growth
stage, and a whole projection.

    python tools/projection_time.py [--resolution 1024] [--batch 16] [--window 0.3] [--windows 5] [--project-images 8] [--steps 200]
                                    [--json out.json]

1. ``ops.pyramid_loss`` (loss + image gradient, and the loss alone) at 256^2 x 1 x 16 and 1024^2 x 3 x 16, beside the same loss and
   gradient composed from torch device ops (an ``avg_pool2d`` chain with autograd) in the same run, alternating.  Bytes: what the
   definition NEEDS -- img and target read once, grad written once (12 bytes per pixel with the gradient, 8 without); the second read of
   the two-pass sizes counts against the kernel.
2. One projection step (forward + loss + sweep + Adam: ``Projector.loss_and_grad`` and ``ops.adam``) at 128^2, 256^2 and 1024^2 with
   ``--batch`` targets, beside ``G.forward`` alone at the same stage and, for orientation, beside the generator step of a training
   iteration (``engine.g_loss_forward`` + ``g_loss_backward`` through an untrained D at the stage's training minibatch).
3. A ``--steps``-step projection of ``--project-images`` images at 256^2 and 1024^2, timed on the host around a device synchronise:
   what ``ProjectionMonitor``'s default period is derived from.

Every shape is warmed first, then timed in ``--windows`` windows of at least ``--window`` seconds of back-to-back calls between two HIP
events; printed: median (min - max).  The weights are untrained.  Needs a GPU; there is no fallback.  Not measured here: data-parallel
runs, Winograd-domain backward forms (the sweep uses the direct backward-data convs only)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def window(fn, seconds, per_call):
    reps = max(3, int(seconds * 1e3 / max(per_call, 1e-3)) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def calibrate(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return window(fn, 0.0, 1e9)


def timed(fns, seconds, windows):
    """{name: (median, min, max) ms per call}; the functions alternate window by window so that all see the same machine."""
    cal = {k: calibrate(f) for k, f in fns.items()}
    w = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            w[k].append(window(f, seconds, cal[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in w.items()}


def torch_pyramid(img, tgt):
    """The same loss and image gradient from torch device ops."""
    x = img.detach().requires_grad_(True)
    p = x - tgt
    total = 0.0
    while True:
        total = total + (p * p).mean(dim=(1, 2, 3))
        if p.shape[-1] == 4:
            break
        p = F.avg_pool2d(p, 2)
    g, = torch.autograd.grad(total.sum(), x)
    return total.detach(), g


def fmt(t):
    return '%9.4f (%8.4f -%8.4f)' % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--project-images', type=int, default=8)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops = pg.ops
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    out = {'window_s': args.window, 'windows': args.windows, 'loss': [], 'step': [], 'projection': []}

    # ---- 1. the loss kernel alone
    print('pyramid loss, ms per call: median (min - max) of %d windows of >= %.1f s' % (args.windows, args.window))
    for N, C, r in ((16, 1, 256), (16, 3, 1024)):
        g = torch.Generator(device=dev).manual_seed(r)
        img = torch.randn(N, C, r, r, device=dev, generator=g)
        tgt = torch.randn(N, C, r, r, device=dev, generator=g)
        scratch = torch.empty(ops.pyramid_scratch_words(N, C, r), device=dev, dtype=torch.float64)
        t = timed({'hip': lambda: ops.pyramid_loss(img, tgt, scratch=scratch),
                   'hip_loss_only': lambda: ops.pyramid_loss(img, tgt, want_grad=False, scratch=scratch),
                   'torch': lambda: torch_pyramid(img, tgt)}, args.window, args.windows)
        l_hip, g_hip = ops.pyramid_loss(img, tgt)
        l_t, g_t = torch_pyramid(img, tgt)
        agree = (float((l_hip - l_t).abs().max() / l_t.abs().max()), float((g_hip - g_t).abs().max() / g_t.abs().max()))
        need, need_lo = 12.0 * img.numel(), 8.0 * img.numel()
        row = {'N': N, 'C': C, 'r': r, 'hip_ms': t['hip'], 'hip_loss_only_ms': t['hip_loss_only'], 'torch_ms': t['torch'],
               'hip_tbs': need / t['hip'][0] / 1e9, 'hip_loss_only_tbs': need_lo / t['hip_loss_only'][0] / 1e9,
               'torch_tbs': need / t['torch'][0] / 1e9, 'torch_over_hip': t['torch'][0] / t['hip'][0], 'max_rel_diff_loss_grad': agree}
        out['loss'].append(row)
        print('  [%d,%d,%d,%d] loss + grad: HIP %s = %.2f TB/s of the %.0f MB the definition needs | loss only %s = %.2f TB/s | torch ops %s'
              ' = %.2f TB/s | torch / HIP %.2fx | largest relative difference loss %.1e grad %.1e'
              % (N, C, r, r, fmt(t['hip']), row['hip_tbs'], need / 1e6, fmt(t['hip_loss_only']), row['hip_loss_only_tbs'], fmt(t['torch']),
                 row['torch_tbs'], row['torch_over_hip'], agree[0], agree[1]), flush=True)
        del img, tgt, scratch, l_hip, g_hip, l_t, g_t

    # ---- 2. one projection step per stage
    torch.manual_seed(1234)
    shape = (1, 3, args.resolution, args.resolution)
    G = pg.Generator(shape).to(dev)
    D = pg.Discriminator(shape).to(dev)
    n = args.batch
    train_mb = {5: 16, 6: 14, 7: 6, 8: 3}                    # DepthManager's default minibatch per depth
    print('one projection step of %d targets, ms: median (min - max)' % n)
    for r in (128, 256, 1024):
        if r > args.resolution:
            continue
        depth = r.bit_length() - 3
        G.depth = D.depth = depth
        G.alpha = D.alpha = 1.0
        g = torch.Generator(device=dev).manual_seed(depth)
        z = torch.randn(n, G.latent_size, device=dev, generator=g)
        targets = torch.rand(n, 3, r, r, device=dev, generator=g) * 2 - 1
        proj = pg.Projector(G)
        m, v = torch.zeros_like(z), torch.zeros_like(z)

        def step():
            _, dz = proj.loss_and_grad(z, targets)
            ops.adam(z.view(-1), dz.view(-1), m.view(-1), v.view(-1), 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.0316)
        mb = train_mb.get(depth, 16)
        zg = torch.randn(mb, G.latent_size, device=dev, generator=g)

        def g_step():
            _, st = pg.engine.g_loss_forward(G, D, zg, pg.engine.WGAN_GP)
            pg.engine.g_loss_backward(st)
        t = timed({'step': step, 'forward': lambda: G.forward(z), 'train_g_step': g_step}, args.window, args.windows)
        row = {'r': r, 'targets': n, 'step_ms': t['step'], 'forward_ms': t['forward'], 'train_g_step_ms': t['train_g_step'],
               'train_minibatch': mb, 'step_over_forward': t['step'][0] / t['forward'][0]}
        out['step'].append(row)
        print('  %4dx%-4d step %s | G.forward alone %s | step / forward %.2fx | G step of a training iteration, minibatch %d (orientation) %s'
              % (r, r, fmt(t['step']), fmt(t['forward']), row['step_over_forward'], mb, fmt(t['train_g_step'])), flush=True)
        G.zero_grad()
        del proj, targets

    # ---- 3. a whole projection
    k = args.project_images
    print('a %d-step projection of %d images, seconds on the host around a device synchronise (second of two runs; the first warms)' % (args.steps, k))
    for r in (256, 1024):
        if r > args.resolution:
            continue
        depth = r.bit_length() - 3
        G.depth, G.alpha = depth, 1.0
        g = torch.Generator(device=dev).manual_seed(100 + depth)
        zstar = torch.randn(k, G.latent_size, device=dev, generator=g)
        targets = G.forward(zstar).clone()
        proj = pg.Projector(G, steps=args.steps)
        secs = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = proj.project(targets)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        ratio = (res.loss / res.history[0]).tolist()
        row = {'r': r, 'images': k, 'steps': args.steps, 'seconds': secs[1], 'first_run_seconds': secs[0], 'ms_per_step': 1e3 * secs[1] / args.steps,
               'final_over_first_loss': ratio}
        out['projection'].append(row)
        print('  %4dx%-4d %.3f s (%.3f ms per step; first run %.3f s) | final / first loss of its own images G(z*): %s'
              % (r, r, secs[1], row['ms_per_step'], secs[0], ['%.3f' % x for x in ratio]), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
