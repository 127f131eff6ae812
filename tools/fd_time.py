#!/usr/bin/env python
"""Device time of the Frechet distance over the random embedding (``metrics.RandomEmbedding``, ``ops.fd_moments_f64``: csrc/embed.hip
with the 3x3 layers of csrc/sampling.hip) against the same result composed from torch's device ops, and against the generator passes
that produce the images.

    python tools/fd_time.py [--shapes 4096x1x256,4096x2x256,4096x3x256,4096x1x64] [--moments 4096x128,30000x128] [--warmup 1]
                            [--runs 5] [--generator-images 512] [--minibatch 16] [--twin 256x1x16,64x1x64] [--no-composed]
                            [--eval 4096x1x256,4096x3x1024] [--json out.json]

A shape is N x C x r: N uint8 images of white noise box-filtered twice, made on the device.  Per shape, between two HIP events, the
median over ``--runs`` spans after ``--warmup`` untimed ones, with the minimum and the maximum as the spread, the paths alternating:
  fused     ``RandomEmbedding(C)(images)`` (chunks of 64) followed by ``ops.fd_moments_f64``
  composed  the same network from torch's device ops in float32 on the same bf16-rounded weights, 64 images at a time: the stem as
            tensor arithmetic, ``F.conv2d``, ``leaky_relu``, the PixelNorm as tensor arithmetic, a cast to bf16 and back per layer,
            ``F.avg_pool2d``, ``mean``; then ``torch.cov`` of the features in float64.  The tool stops if the features of the two
            paths differ by more than 2^-5 anywhere (one bf16 ulp at 4, what a rounding that falls the other way can move).
  generator ``G.forward`` of a default ``pg.Generator`` of that resolution on ``--generator-images`` latents, ``--minibatch`` at a
            time, in wall-clock time around device synchronisations, scaled to N images.
``--moments`` M x F: ``ops.fd_moments_f64`` alone on random features; the rate is 2 M F^2 / time (the arithmetic of the full matrix;
the kernel computes the tiles on or above the diagonal only).  ``--twin``: the largest difference between device features and the
host twin's.  ``--eval`` N x C x r: one ``metrics.FrechetDistance`` evaluation the way ``plugins.FDMonitor`` runs it, in wall-clock
time around device synchronisations: ``fit()`` on min(N, 1024) random reals, ``--generator-images`` samples of a default generator
``--minibatch`` at a time without and with ``feed`` (the difference is the metric's feed: quantise, reduce above 256^2, embed),
``result()``; per-image figures, scaled to N samples.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def span(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def timed(fns, warmup, runs):
    """(median, min, max) milliseconds per call of every function of ``fns``, the functions alternating span by span."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(runs):
        events = [span(fn) for fn in fns]
        torch.cuda.synchronize()
        for t, (a, b) in zip(times, events):
            t.append(a.elapsed_time(b))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def box_images(n, C, r, dev, g, passes=2):
    x = torch.rand((n, C, r, r), device=dev, generator=g) - 0.5
    for _ in range(passes):
        x = 3.0 * sum(torch.roll(x, (dy, dx), (2, 3)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    return ((x + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8)


def composed_features(emb, images, metrics):
    out = []
    for s in range(0, images.shape[0], 64):
        u8 = images[s:s + 64]
        x = ((u8.float() - 127.5) / 127.5).to(torch.bfloat16).float()
        H = int(u8.shape[-1])
        for H, cin, _ in emb.layers(H):
            w = emb.weights(H, cin).float().permute(2, 3, 0, 1)[:, :x.shape[1]]
            v = F.leaky_relu(F.conv2d(x, w, None, 1, 1) * (2.0 / (9 * cin)) ** 0.5, metrics.EMBED_SLOPE)
            x = (v * torch.rsqrt(v.pow(2).mean(dim=1, keepdim=True) + metrics.EMBED_EPS)).to(torch.bfloat16).float()
            if H > 4:
                x = F.avg_pool2d(x, 2).to(torch.bfloat16).float()
        out.append(x.mean(dim=(2, 3)))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x1x256,4096x2x256,4096x3x256,4096x1x64')
    ap.add_argument('--moments', default='4096x128,30000x128')
    ap.add_argument('--twin', default='256x1x16,64x1x64')
    ap.add_argument('--eval', default='4096x1x256,4096x3x1024')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--generator-images', type=int, default=512)
    ap.add_argument('--minibatch', type=int, default=16)
    ap.add_argument('--no-composed', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops, metrics = pg.ops, pg.metrics
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    print('%s, torch %s; FD_SLICE = %d, FD_TILE = %d' % (torch.cuda.get_device_name(dev), torch.__version__, ops.FD_SLICE, ops.FD_TILE))
    g = torch.Generator(device=dev).manual_seed(1)
    rows, moments, twins = [], [], []
    for shape in [s for s in args.moments.split(',') if s]:
        M, Fdim = (int(v) for v in shape.split('x'))
        x = torch.randn((M, Fdim), device=dev, generator=g)
        (t,) = timed([lambda: ops.fd_moments_f64(x)], max(1, args.warmup), args.runs)
        (tc,) = timed([lambda: (x.double().mean(dim=0), torch.cov(x.double().t()))], max(1, args.warmup), args.runs)
        rate = 2.0 * M * Fdim * Fdim / (t[0] * 1e-3)
        moments.append({'M': M, 'F': Fdim, 'ms': t, 'torch_cov_ms': tc, 'flops_per_s': rate})
        print('moments %6d x %3d: %.4f ms (%.4f-%.4f), %.3f Tflop/s fp64 by 2 M F^2; torch mean + cov in float64 %.4f ms (%.4f-%.4f)'
              % (M, Fdim, t[0], t[1], t[2], rate / 1e12, tc[0], tc[1], tc[2]), flush=True)
    for shape in [s for s in args.shapes.split(',') if s]:
        N, C, r = (int(v) for v in shape.split('x'))
        images = box_images(N, C, r, dev, g)
        emb = metrics.RandomEmbedding(C)
        row = {'N': N, 'C': C, 'r': r}

        def fused():
            return ops.fd_moments_f64(emb(images))

        def composed():
            f = composed_features(emb, images, metrics).double()
            return f.mean(dim=0), torch.cov(f.t())

        fns = [fused]
        if not args.no_composed:
            d = float((composed_features(emb, images[:256], metrics) - emb(images[:256])).abs().max())
            if not d <= 2.0 ** -5:
                raise SystemExit('%s: the features of the two paths differ by %.3e: nothing timed' % (shape, d))
            row['composed_feature_difference'] = d
            fns.append(composed)
        res = timed(fns, args.warmup, args.runs)
        row['fused_ms'] = res[0]
        if not args.no_composed:
            row['composed_ms'] = res[1]
        feats = emb(images)
        row['outside_-1_3'] = float(((feats < -1) | (feats > 3)).float().mean())
        row['feature_range'] = (float(feats.min()), float(feats.max()))
        torch.manual_seed(3)
        G = pg.Generator((1, C, r, r)).to(dev)
        G.depth = G.max_depth                                                # the full resolution
        n_g = min(N, args.generator_images)
        z = torch.randn((args.minibatch, G.latent_size), device=dev)
        best = None
        for _ in range(2):                                                   # the first round warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                for s in range(0, n_g, args.minibatch):
                    G.forward(z[:min(args.minibatch, n_g - s)])
            torch.cuda.synchronize()
            best = (time.perf_counter() - t0) * N / n_g
        row['generator_s_for_N'] = best
        row['generator_images_timed'] = n_g
        rows.append(row)
        print('%d x %d x %d^2: embedding + moments %.2f ms (%.2f-%.2f)%s; generator passes %.2f s for %d images (timed %d, batches of %d); '
              'features in [%.2f, %.2f], %.4f%% outside (-1, 3)'
              % (N, C, r, res[0][0], res[0][1], res[0][2],
                 '' if args.no_composed else ', composed from torch ops %.2f ms (%.2f-%.2f), ratio %.2f, feature difference %.2e'
                 % (res[1][0], res[1][1], res[1][2], res[1][0] / res[0][0], row['composed_feature_difference']),
                 best, N, n_g, args.minibatch, row['feature_range'][0], row['feature_range'][1], 100 * row['outside_-1_3']), flush=True)
        del images, emb, G, feats
        torch.cuda.empty_cache()
    for shape in [s for s in args.twin.split(',') if s]:
        N, C, r = (int(v) for v in shape.split('x'))
        images = box_images(N, C, r, dev, g)
        d = (metrics.RandomEmbedding(C)(images).cpu() - metrics.RandomEmbedding(C, device='cpu')(images.cpu())).abs()
        twins.append({'N': N, 'C': C, 'r': r, 'max': float(d.max()), 'mean': float(d.mean()), 'share_different': float((d > 0).float().mean())})
        print('%d x %d x %d^2: device features against the host twin: largest difference %.3e, mean %.3e, %.2f%% of the features differ'
              % (N, C, r, twins[-1]['max'], twins[-1]['mean'], 100 * twins[-1]['share_different']), flush=True)
    evals = []
    for shape in [s for s in args.eval.split(',') if s]:
        N, C, r = (int(v) for v in shape.split('x'))
        n_real, n_g = min(N, 1024), min(N, args.generator_images)
        stack = torch.randint(0, 256, (n_real, C, r, r), dtype=torch.uint8, device=dev, generator=g)
        metric = metrics.FrechetDistance(stack)
        torch.manual_seed(3)
        G = pg.Generator((1, C, r, r)).to(dev)
        G.depth = G.max_depth
        z = torch.randn((args.minibatch, G.latent_size), device=dev)
        with torch.no_grad():
            if tuple(G.forward(z).shape) != (args.minibatch, C, r, r):
                raise SystemExit('%s: the generator does not run at the full resolution: nothing timed' % shape)
        best = None
        for _ in range(2):                                                   # the first round warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metric.fit()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            with torch.no_grad():
                for s in range(0, n_g, args.minibatch):
                    G.forward(z)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            with torch.no_grad():
                for s in range(0, n_g, args.minibatch):
                    metric.feed(G.forward(z))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            res = metric.result()
            t4 = time.perf_counter()
            best = ((t1 - t0) / n_real, (t2 - t1) / n_g, (t3 - t2) / n_g, t4 - t3)
        evals.append({'N': N, 'C': C, 'r': r, 'reals_timed': n_real, 'images_timed': n_g, 'fit_s_per_real': best[0],
                      'generator_s_per_image': best[1], 'generator_and_feed_s_per_image': best[2], 'result_s': best[3], 'fd': res['fd']})
        print('evaluation at %d x %d^2, batches of %d: fit %.3f ms per real (%d timed), generator %.3f ms per image, generator + feed '
              '%.3f ms per image (%d timed), result %.4f s; for %d samples: generator %.2f s, feed %.2f s'
              % (C, r, args.minibatch, 1e3 * best[0], n_real, 1e3 * best[1], 1e3 * best[2], n_g, best[3], N, N * best[1],
                 N * (best[2] - best[1])), flush=True)
        del stack, metric, G
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'runs': args.runs, 'warmup': args.warmup, 'moments': moments, 'rows': rows,
                       'twin': twins, 'evaluations': evals}, f, indent=1)


if __name__ == '__main__':
    main()
