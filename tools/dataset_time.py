#!/usr/bin/env python
"""Device time of one real-image batch of DeviceImageDataset (one launch of pg_real_batch_u8), per growth stage, against the
composition it replaces: ``stack.index_select`` + ``ops.pyramid_level_u8`` + ``torch.flip`` + ``ops.real_prepare_u8``.

    python tools/dataset_time.py [--resolution 1024] [--images 64] [--channels 3] [--alpha 0.5] [--warmup 3] [--runs 9] [--inner 20]
                                 [--footprint-images 0] [--json out.json]

For every stage 4x4 .. ``--resolution`` at the reference's minibatch sizes (16; 14 / 6 / 3 from 256x256 on: DepthManager's
defaults), for both pyramid modes and with and without mirror flags, ``--inner`` batches are issued between two HIP events; the
figure printed is the median over ``--runs`` such spans after ``--warmup`` untimed ones, divided by ``--inner``.  The two paths are
run alternately and compared bitwise first: the tool stops if they differ.  ``--alpha`` < 1 keeps the fade in both.  The last
column is the bytes the fused launch has to move (source bytes read + fp32 written) over its time.  ``--footprint-images N``
additionally allocates an N-image stack of ``--resolution`` in both pyramid modes and reports ``torch.cuda.memory_allocated``
(N = 30000 at 1024x1024x3 is 94 GB + 1/3).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

MINIBATCH_DEFAULT, MINIBATCH_OVERRIDES = 16, {6: 14, 7: 6, 8: 3}


def span(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--footprint-images', type=int, default=0)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops = pg.ops
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    R, M, C = args.resolution, args.images, args.channels
    top = R.bit_length() - 1
    print('%s, torch %s; %d images x %d x %dx%d uint8, alpha %.2f' % (torch.cuda.get_device_name(dev), torch.__version__, M, C, R, R, args.alpha))
    images = torch.randint(0, 256, (M, C, R, R), dtype=torch.uint8, generator=torch.Generator().manual_seed(R + C))
    rows = []
    print('%-6s %-7s %-6s %3s %12s %14s %8s %10s' % ('stage', 'pyramid', 'mirror', 'n', 'batch() us', 'composition us', 'ratio', 'GB/s'))
    for pyramid in ('chain', 'direct'):
        ds = pg.DeviceImageDataset(images, pyramid=pyramid, mirror_augment=True, alpha=args.alpha, device=dev)
        for depth in range(0, top - 1):
            ds.model_depth = depth
            r = 4 * 2 ** depth
            n = MINIBATCH_OVERRIDES.get(depth, MINIBATCH_DEFAULT)
            stack, _, dd = ds._stage()
            for mirror in (False, True):
                idx, flip = ds.draw_indices(n)
                idx, flip = idx.clone(), (flip.clone() if mirror else None)
                flip_b = None if flip is None else flip.bool().view(-1, 1, 1, 1)

                def fused():
                    return ops.real_batch_u8(stack, idx, flip, dd, args.alpha, ds.range_in, ds.range_out)

                def composed():
                    level = stack.index_select(0, idx)
                    if dd:
                        level = ops.pyramid_level_u8(level, dd, ds.range_in)
                    if flip_b is not None:
                        level = torch.where(flip_b, torch.flip(level, dims=[-1]), level)
                    return ops.real_prepare_u8(level, args.alpha, ds.range_in, ds.range_out)
                if not torch.equal(fused(), composed()):
                    raise SystemExit('stage %d %s mirror=%s: the fused batch and the composition differ: nothing timed' % (r, pyramid, mirror))
                for _ in range(args.warmup):
                    span(fused, args.inner)
                    span(composed, args.inner)
                torch.cuda.synchronize()
                t_f, t_c = [], []
                for _ in range(args.runs):                                   # alternating, so that both see the same machine
                    ef, ec = span(fused, args.inner), span(composed, args.inner)
                    torch.cuda.synchronize()
                    t_f.append(ef[0].elapsed_time(ef[1]) * 1e3 / args.inner)
                    t_c.append(ec[0].elapsed_time(ec[1]) * 1e3 / args.inner)
                f_us, c_us = statistics.median(t_f), statistics.median(t_c)
                moved = n * C * r * r * ((1 if dd == 0 else 4) + 4)
                rows.append({'stage': r, 'pyramid': pyramid, 'mirror': mirror, 'n': n, 'depthdiff': dd, 'batch_us': f_us, 'composition_us': c_us,
                             'batch_us_min_max': [min(t_f), max(t_f)], 'composition_us_min_max': [min(t_c), max(t_c)],
                             'bytes': moved, 'gb_per_s': moved / f_us / 1e3})
                print('%-6d %-7s %-6s %3d %12.2f %14.2f %8.2f %10.1f' % (r, pyramid, 'yes' if mirror else 'no', n, f_us, c_us, c_us / f_us, moved / f_us / 1e3))
        ds.close()
    footprint = {}
    if args.footprint_images > 0:
        del images
        for pyramid in ('chain', 'direct'):
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated(dev)
            big = torch.empty((args.footprint_images, C, R, R), dtype=torch.uint8, device=dev)   # (contents do not matter for the footprint)
            ds = pg.DeviceImageDataset.__new__(pg.DeviceImageDataset)
            ds.range_in = (0, 255)
            levels = {top: big}
            if pyramid == 'chain':
                for depth in range(top - 1, 1, -1):
                    levels[depth] = ds._level_below(levels[depth + 1])
            torch.cuda.synchronize()
            footprint[pyramid] = torch.cuda.memory_allocated(dev) - before
            print('footprint %-7s %d images: %.3f GB' % (pyramid, args.footprint_images, footprint[pyramid] / 1e9))
            del levels, big, ds
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'resolution': R, 'images': M, 'channels': C, 'alpha': args.alpha, 'runs': args.runs,
                       'warmup': args.warmup, 'inner': args.inner, 'rows': rows, 'footprint_bytes': footprint}, f, indent=1)


if __name__ == '__main__':
    main()
