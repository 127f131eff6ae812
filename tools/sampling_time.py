#!/usr/bin/env python
"""Device time of the generator's forward pass per growth stage, fp32 (``G.forward``) against bf16 (``sampling.Sampler``), with the image
deviation per stage and the metric neutrality at 256x256 (docs/experiments_sampling.md).

    python tools/sampling_time.py [--resolution 1024] [--batch 16] [--window 0.3] [--windows 5] [--metrics-depth 6] [--json out.json]

Both passes run on the same seeded network in the same process.  Every stage is warmed first, then timed in ``--windows`` pairs of
windows, fp32 and bf16 alternating, each window at least ``--window`` seconds of back-to-back calls between two HIP events.  Printed per
stage: the median time per call and its min - max over the windows, the speed-up, the FLOP/s and bytes/s each pass achieves on the
operations and bytes the layer table NEEDS (counted below from the shapes: the convolutions' multiply-adds; every activation written
once and read once at the pass's width, the weights once, the image once -- what a pass really moves on top of that, such as the fp32
scratch of an unfused PixelNorm, counts against it), and the share of the bound that applies: the larger of FLOP / peak rate and bytes
/ peak bandwidth.  Then the deviation of the bf16 images from the fp32 ones on the same latents (relative L2, largest difference,
share of uint8 levels that change), and at ``--metrics-depth``: MS-SSIM of the same 64 latent pairs under both precisions, the sliced
Wasserstein distance between the fp32 and the bf16 images of the same 2048 latents, and between two fp32 sets of different latents
(the metric's own noise floor).  The weights are untrained.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_BF16, PEAK_F32, PEAK_HBM = 2.5e15, 157.3e12, 8.0e12       # dense MFMA rates and HBM bandwidth of the MI355X (spec)


def stage_work(G, depth, alpha, n, width):
    """(FLOP, bytes) a pass of n images needs at ``width`` bytes per stored activation element."""
    C, L = G.num_channels, G.latent_size
    b0 = G.block0
    flop = 2 * 16 * L * b0.c1.ch_out
    byts = 16 * L * b0.c1.ch_out * 4 / n + L * 4 + 16 * b0.c1.ch_out * width          # block 0 c1: fp32 weights once per batch
    layers = [(b0.c2, 4, 4)]
    H = 4
    for i in range(depth):
        blk = G.blocks[i]
        layers += [(blk.c1, H, 2 * H), (blk.c2, 2 * H, 2 * H)]
        H *= 2
    for lay, hin, hout in layers:
        flop += 2 * 9 * lay.cin_store * lay.ch_out * hout * hout
        byts += hin * hin * lay.cin_store * width + hout * hout * lay.ch_out * width + 9 * lay.cin_store * lay.ch_out * width / n
    last = layers[-1][0].ch_out
    flop += 2 * C * last * H * H
    byts += H * H * last * width + C * H * H * 4
    if depth and alpha < 1.0:
        prev = layers[-2][0].cin_store
        flop += 2 * C * prev * H * H
        byts += (H // 2) ** 2 * prev * width
    return n * flop, n * byts


def window(fn, seconds, per_call):
    """Back-to-back calls for at least ``seconds`` (from the calibrated time per call) between two events -> ms per call."""
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


def layer_times(G, S, z, runs=5):
    """The bf16 pass at the last stage, layer by layer: every 3x3 layer (its one or two launches) between two events, median of ``runs``."""
    G.depth, G.alpha = G.max_depth, 1.0
    real, spans = S._layer, []

    def bracketed(x, lay, N, H, ups=False):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = real(x, lay, N, H, ups=ups)
        b.record()
        spans.append((lay, H, a, b))
        return y
    S._layer = bracketed
    try:
        per_run = []
        for _ in range(runs + 1):
            del spans[:]
            S.forward(z)
            torch.cuda.synchronize()
            per_run.append([a.elapsed_time(b) for _, _, a, b in spans])
        table = []
        print('bf16 pass at the last stage, per 3x3 layer (median of %d; an event pair around each layer, so launch gaps are inside)' % runs)
        print('%6s %10s %10s %12s %10s' % ('H', 'channels', 'ms', 'TFLOP/s', 'GB/s'))
        for i, (lay, H, _, _) in enumerate(spans):
            ms = statistics.median(r[i] for r in per_run[1:])
            hin = H // 2 if i and i % 2 else H
            n = z.shape[0]
            flop = 2 * 9 * lay.cin_store * lay.ch_out * H * H * n
            byts = n * (hin * hin * lay.cin_store + H * H * lay.ch_out) * 2 + 9 * lay.cin_store * lay.ch_out * 2
            table.append({'H': H, 'cin': lay.cin_store, 'cout': lay.ch_out, 'ms': ms, 'tflops': flop / ms / 1e9, 'gbs': byts / ms / 1e6})
            print('%6d %4d->%4d %10.4f %12.1f %10.1f' % (H, lay.cin_store, lay.ch_out, ms, flop / ms / 1e9, byts / ms / 1e6))
        return table
    finally:
        del S._layer


def levels(img, drange=(-1, 1)):
    lo, hi = drange
    return ((img - lo) * (255.0 / (hi - lo))).round().clamp(0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--metrics-depth', type=int, default=6)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    pg.ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    torch.manual_seed(1234)
    G = pg.Generator((1, 3, args.resolution, args.resolution)).to(dev)
    S = pg.sampler_for(G)
    n = args.batch
    z = torch.randn(n, G.latent_size, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    rows = []
    print('%d images per call, untrained weights; windows of >= %.1f s, median of %d (min - max)' % (n, args.window, args.windows))
    print('%5s %28s %28s %8s | %21s | %21s | %s' % ('stage', 'fp32 ms', 'bf16 ms', 'speed-up', 'fp32 TFLOP/s  TB/s', 'bf16 TFLOP/s  TB/s',
                                                    'bf16 share of its bound'))
    for depth in range(G.max_depth + 1):
        G.depth, G.alpha = depth, 1.0
        R = 4 << depth
        f32, b16 = (lambda: G.forward(z)), (lambda: S.forward(z))
        t32, t16 = calibrate(f32), calibrate(b16)
        w32, w16 = [], []
        for _ in range(args.windows):                                       # alternating, so that both see the same machine
            w32.append(window(f32, args.window, t32))
            w16.append(window(b16, args.window, t16))
        m32, m16 = statistics.median(w32), statistics.median(w16)
        flop, by32 = stage_work(G, depth, 1.0, n, 4)
        _, by16 = stage_work(G, depth, 1.0, n, 2)
        bound16 = max(flop / PEAK_BF16, by16 / PEAK_HBM)
        bound32 = max(flop / PEAK_F32, by32 / PEAK_HBM)
        which16 = 'MFMA' if flop / PEAK_BF16 >= by16 / PEAK_HBM else 'HBM'
        which32 = 'MFMA' if flop / PEAK_F32 >= by32 / PEAK_HBM else 'HBM'
        a, b = G.forward(z), S.forward(z)
        diff = (b - a).double()
        dev_row = {'rel_l2': float(diff.norm() / a.double().norm()), 'max': float(diff.abs().max()), 'rms_fp32': float(a.double().pow(2).mean().sqrt()),
                   'levels_changed': float((levels(a) != levels(b)).double().mean())}
        row = {'stage': R, 'depth': depth, 'fp32_ms': m32, 'fp32_min': min(w32), 'fp32_max': max(w32), 'bf16_ms': m16, 'bf16_min': min(w16),
               'bf16_max': max(w16), 'speedup': m32 / m16, 'clear_of_spread': min(w32) > max(w16), 'flop': flop, 'bytes_fp32': by32,
               'bytes_bf16': by16, 'fp32_tflops': flop / m32 / 1e9, 'bf16_tflops': flop / m16 / 1e9, 'fp32_tbs': by32 / m32 / 1e9,
               'bf16_tbs': by16 / m16 / 1e9, 'bf16_bound': which16, 'bf16_share': bound16 * 1e3 / m16, 'fp32_bound': which32,
               'fp32_share': bound32 * 1e3 / m32, 'deviation': dev_row}
        rows.append(row)
        print('%5d %10.4f (%8.4f -%8.4f) %10.4f (%8.4f -%8.4f) %7.2fx | %10.1f %9.3f | %10.1f %9.3f | %5.1f %% of %s (fp32: %5.1f %% of %s)'
              % (R, m32, min(w32), max(w32), m16, min(w16), max(w16), m32 / m16, row['fp32_tflops'], row['fp32_tbs'], row['bf16_tflops'],
                 row['bf16_tbs'], 100 * row['bf16_share'], which16, 100 * row['fp32_share'], which32), flush=True)
    print('deviation of the bf16 images from the fp32 images of the same latents')
    print('%5s %12s %12s %12s %16s' % ('stage', 'rel L2', 'max |diff|', 'rms (fp32)', 'levels changed'))
    for r in rows:
        d = r['deviation']
        print('%5d %12.4e %12.4e %12.4f %15.2f %%' % (r['stage'], d['rel_l2'], d['max'], d['rms_fp32'], 100 * d['levels_changed']))

    out = {'batch': n, 'window_s': args.window, 'windows': args.windows, 'stages': rows}
    out['layers'] = layer_times(G, S, z)
    md = min(args.metrics_depth, G.max_depth)
    if md >= 2:
        G.depth, G.alpha = md, 1.0
        R = 4 << md
        g = torch.Generator(device=dev).manual_seed(2)
        lat = lambda k: torch.randn(k, G.latent_size, device=dev, generator=g)
        ms = {p: pg.metrics.MultiScaleSSIM(R, 64, num_channels=3) for p in ('fp32', 'bf16')}
        for _ in range(64 // n):
            za, zb = lat(n), lat(n)
            ms['fp32'].feed(G.forward(za), G.forward(zb))
            ms['bf16'].feed(S.forward(za), S.forward(zb))
        res = {p: m.result() for p, m in ms.items()}
        print('MS-SSIM of the same 64 latent pairs at %dx%d: fp32 %.6f (std %.6f), bf16 %.6f (std %.6f), difference %.2e'
              % (R, R, res['fp32']['msssim'], res['fp32']['std'], res['bf16']['msssim'], res['bf16']['std'],
                 res['bf16']['msssim'] - res['fp32']['msssim']))
        swd_same = pg.metrics.SlicedWasserstein(R, 2048)
        swd_floor = pg.metrics.SlicedWasserstein(R, 2048)
        for _ in range(2048 // n):
            za, zb = lat(n), lat(n)
            a = G.forward(za)
            swd_same.feed_real(a)
            swd_same.feed_fake(S.forward(za))
            swd_floor.feed_real(a)
            swd_floor.feed_fake(G.forward(zb))
        same, floor = swd_same.result(), swd_floor.result()
        print('SWD x 1e3 at %dx%d, 2048 images: fp32 against bf16 on the same latents %s (mean %.4f); fp32 against fp32 on other latents %s '
              '(mean %.4f): the noise floor' % (R, R, ['%.4f' % v for v in same['swd']], same['mean'], ['%.4f' % v for v in floor['swd']],
                                                floor['mean']))
        out['metrics'] = {'resolution': R, 'msssim_fp32': res['fp32']['msssim'], 'msssim_bf16': res['bf16']['msssim'],
                          'msssim_std_fp32': res['fp32']['std'], 'msssim_std_bf16': res['bf16']['std'], 'swd_levels': same['levels'],
                          'swd_same_latents': same['swd'], 'swd_same_latents_mean': same['mean'], 'swd_noise_floor': floor['swd'],
                          'swd_noise_floor_mean': floor['mean']}
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
