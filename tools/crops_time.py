#!/usr/bin/env python
"""Device time of one crop batch of DeviceStripDataset (one launch of pg_crop_batch_u8) at the training shapes, against its two
yardsticks, and the bytes a strip level takes.

    python tools/crops_time.py [--alpha 0.5] [--warmup 3] [--runs 9] [--inner 50] [--json out.json]

Shapes: 16 x 3 x 1024^2, 16 x 2 x 512^2, 64 x 1 x 128^2 (n x C x R^2), four strips of 3R, 5R, 4R and 6R + 37 columns.  Modes:
'source' (chain or direct at the source resolution: shift 0, depthdiff 0), 'chain-3' (the stored level three stages down: S = R/8,
shift 3) and 'direct-3' (the source level with depthdiff 3).  Start columns: 'aligned' (multiples of 16 at the level read) and 'odd'.

  floor        ``ops.real_batch_u8`` on the same windows materialised beforehand as a stack [n,C,S,S]: aligned rows, no gather.
  composition  the windows materialised per batch with torch device ops -- one slice per image from host-known positions,
               ``torch.stack`` -- and then ``ops.real_batch_u8``.

``--inner`` batches are issued between two HIP events; a figure is the median over ``--runs`` such spans after ``--warmup`` untimed
ones, divided by ``--inner``.  The three are run alternately and compared bitwise first: the tool stops if they differ.  Needs a GPU;
there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = ((16, 3, 1024), (16, 2, 512), (64, 1, 128))
WIDTHS = (3, 5, 4, 6)


def span(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops = pg.ops
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    print('%s, torch %s, library %s; alpha %.2f' % (torch.cuda.get_device_name(dev), torch.__version__, pg.LIB_PATH, args.alpha))
    rows, memory = [], []
    print('%-14s %-9s %-8s %10s %10s %14s %8s %8s %9s' % ('n x C x R', 'mode', 'starts', 'crop us', 'floor us', 'composition us', '/floor', 'comp/', 'GB/s'))
    for n, C, R in SHAPES:
        g = torch.Generator().manual_seed(R + C)
        strips = [torch.randint(0, 256, (C, R, w * R + (37 if w == WIDTHS[-1] else 0)), dtype=torch.uint8, generator=g) for w in WIDTHS]
        ds = pg.DeviceStripDataset(strips, pyramid='chain', model_dataset_depth_offset=2, mirror_augment=True, alpha=args.alpha, device=dev)
        top = ds.max_dataset_depth
        payload = sum(C * R * t for t in ds.lengths)
        for depth, b in sorted(ds.level_bytes().items(), reverse=True):
            k = top - depth
            memory.append({'C': C, 'R': R, 'level': k, 'bytes': b, 'payload_bytes': payload >> (2 * k), 'source_payload_bytes': payload})
        total = sum(ds.level_bytes().values())
        print('  memory %dx%d^2: source level %d B for sum C R T = %d B (x%.4f); all %d levels of the chain %d B (x%.4f)'
              % (C, R, ds.level_bytes()[top], payload, ds.level_bytes()[top] / payload, len(ds.level_bytes()), total, total / payload))
        gen = torch.Generator().manual_seed(7)
        for mode, depth, shift, dd in (('source', top, 0, 0), ('chain-3', top - 3, 3, 0), ('direct-3', top, 0, 3)):
            level = ds._levels[depth]
            S = level.S
            for starts in ('aligned', 'odd'):
                idx_h = torch.randint(0, len(strips), (n,), generator=gen)
                room = torch.tensor([level.cols[m] - S for m in idx_h.tolist()])
                u_h = torch.minimum((torch.rand(n, generator=gen, dtype=torch.float64) * (room + 1)).long(), room)
                if starts == 'aligned':
                    u_h = (u_h // 16) * 16
                else:
                    u_h = u_h | 1
                    u_h = torch.where(u_h > room, u_h - 2, u_h)
                assert bool((u_h >= 0).all()) and bool((u_h <= room).all()) and bool(((u_h % 16 == 0) if starts == 'aligned' else (u_h % 2 == 1)).all())
                pos_h = u_h << shift
                flip_h = torch.randint(0, 2, (n,), generator=gen, dtype=torch.uint8)
                idx, pos, flip = idx_h.to(dev), pos_h.to(dev), flip_h.to(dev)
                arange = torch.arange(n, device=dev)
                pairs = list(zip(idx_h.tolist(), u_h.tolist()))

                def materialise():
                    return torch.stack([level.strip(m)[:, :, u:u + S] for m, u in pairs])
                stack = materialise()

                def crop():
                    return ops.crop_batch_u8(level, idx, pos, flip, shift, dd, args.alpha, ds.range_in, ds.range_out)

                def floor():
                    return ops.real_batch_u8(stack, arange, flip, dd, args.alpha, ds.range_in, ds.range_out)

                def composed():
                    return ops.real_batch_u8(materialise(), arange, flip, dd, args.alpha, ds.range_in, ds.range_out)
                want = floor()
                if not (torch.equal(crop(), want) and torch.equal(composed(), want)):
                    raise SystemExit('%dx%dx%d^2 %s %s: the crop batch, the floor and the composition differ: nothing timed' % (n, C, R, mode, starts))
                fns = (crop, floor, composed)
                for _ in range(args.warmup):
                    for fn in fns:
                        span(fn, args.inner)
                torch.cuda.synchronize()
                times = [[], [], []]
                for _ in range(args.runs):                                   # alternating, so that all three see the same machine
                    evs = [span(fn, args.inner) for fn in fns]
                    torch.cuda.synchronize()
                    for t, e in zip(times, evs):
                        t.append(e[0].elapsed_time(e[1]) * 1e3 / args.inner)
                c_us, f_us, m_us = (statistics.median(t) for t in times)
                r = S >> dd
                moved = n * C * (S * S if dd == 0 else 4 * r * r) + n * C * r * r * 4     # source bytes needed + fp32 written
                rows.append({'n': n, 'C': C, 'R': R, 'mode': mode, 'S': S, 'shift': shift, 'depthdiff': dd, 'starts': starts, 'crop_us': c_us,
                             'floor_us': f_us, 'composition_us': m_us, 'min_max_us': [[min(t), max(t)] for t in times], 'bytes': moved,
                             'gb_per_s': moved / c_us / 1e3})
                print('%-14s %-9s %-8s %10.2f %10.2f %14.2f %8.2f %8.2f %9.1f'
                      % ('%dx%dx%d^2' % (n, C, R), mode, starts, c_us, f_us, m_us, c_us / f_us, m_us / c_us, moved / c_us / 1e3))
        ds.close()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'library': pg.LIB_PATH, 'alpha': args.alpha, 'runs': args.runs, 'warmup': args.warmup,
                       'inner': args.inner, 'rows': rows, 'memory': memory}, f, indent=1)


if __name__ == '__main__':
    main()
