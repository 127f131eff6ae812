#!/usr/bin/env python
"""Device time and peak memory of one shift-invariant window search (``ops.shift_l2min_u8``: pg_shift_l2min_u8, every start column of
every strip, nothing of size queries x starts stored) against the composition that existed before it: the overlapping windows
materialised chunk by chunk with torch (``unfold`` + ``contiguous``), ``ops.l2dist_u8`` on each chunk, and the same keys taken from
the distances with torch ops.

    python tools/shiftnn_time.py [--shapes 10x75000x2x256x64,10x75000x2x1024x64] [--warmup 1] [--runs 3] [--chunk-mb 1024] [--json out.json]

A shape is strips x columns x C x S x K (10 x 75000 columns is 10 minutes at hop 128 and 16 kHz).  The strips and the queries are
random bytes made on the device; query 0 is the window at an odd start of the last strip.  Before anything is timed the keys of the
two paths must be equal bit for bit and the planted copy must come back at distance 0 at its start: the tool stops otherwise.  Every
figure is the median over ``--runs`` spans between two HIP events after ``--warmup`` untimed ones, the two paths alternating.
Rate = 2 K starts C S S integer operations / time, against the int8 MFMA dense peak (twice the ~2.5 PF BF16 rate of the data sheet).
Peak memory = ``torch.cuda.max_memory_allocated`` of a call above what is resident before it (the level and the queries).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

INT8_PEAK = 5.0e15


def timed(fns, warmup, runs):
    """(median, min, max) milliseconds per call of every function of ``fns``, the functions alternating call by call."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(runs):
        events = []
        for fn in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events.append((a, b))
        torch.cuda.synchronize()
        for t, (a, b) in zip(times, events):
            t.append(a.elapsed_time(b))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def peak_above_resident(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10x75000x2x256x64,10x75000x2x1024x64')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=1024, help='bytes of one chunk of materialised windows of the composition')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import pggan_amd as pg
    ops = pg.ops
    ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    print('%s, torch %s; SHIFT_MAX_QUERIES = %d, chunk %d MiB' % (torch.cuda.get_device_name(dev), torch.__version__, ops.SHIFT_MAX_QUERIES,
                                                                  args.chunk_mb))
    print('%-26s %4s %12s %12s %7s %10s %8s %12s %12s' % ('level', 'K', 'shift ms', 'windows ms', 'ratio', 'int8 TOPS', '% peak',
                                                         'shift MiB', 'windows MiB'))
    rows = []
    g = torch.Generator(device=dev).manual_seed(1)
    for shape in args.shapes.split(','):
        M, T, C, S, K = (int(v) for v in shape.split('x'))
        D, seg = C * S * S, S
        level = pg.dataset.StripLevel.empty(C, S, [T] * M, dev)
        for m in range(M):
            level.strip(m).copy_(torch.randint(0, 256, (C, S, T), dtype=torch.uint8, device=dev, generator=g))
        queries = torch.randint(0, 256, (K, C, S, S), dtype=torch.uint8, device=dev, generator=g)
        u_star = (T - S) // 2 | 1
        queries[0].copy_(level.strip(M - 1)[:, :, u_star:u_star + S])
        seg_strip, seg_start, first = ops.shift_segments(level.cols, S, seg)
        ops.shift_table(level, seg)                                          # (built once per level, as a monitor would have it)
        n = T - S + 1
        step = max(1, (args.chunk_mb << 20) // D // seg) * seg               # starts per chunk: whole segments
        offs = torch.arange(seg, device=dev, dtype=torch.int64)

        def shift():
            return ops.shift_l2min_u8(level, queries, seg)

        def windows():
            keys = []
            for m in range(M):
                win = level.strip(m).unfold(2, S, 1).permute(2, 0, 1, 3)     # [n,C,S,S]: a view, nothing copied yet
                for a in range(0, n, step):
                    chunk = win[a:a + step].contiguous()                     # the materialised windows of this chunk
                    d = ops.l2dist_u8(chunk, queries)                        # [K, w]
                    w = d.shape[1]
                    full = w // seg * seg
                    if full:
                        keys.append(((d[:, :full].view(K, -1, seg) << ops.SHIFT_POS_BITS) + offs).min(dim=2)[0])
                    if w > full:
                        keys.append(((d[:, full:] << ops.SHIFT_POS_BITS) + offs[:w - full]).min(dim=1, keepdim=True)[0])
                    del chunk, d
            return torch.cat(keys, dim=1)

        # exactness first
        key = shift()
        if not torch.equal(key, windows()):
            raise SystemExit('%s: the keys of the two paths differ: nothing timed' % shape)
        gstar = int(first[M - 1]) + u_star // seg
        if int(key[0, gstar]) != u_star % seg:
            raise SystemExit('%s: the planted copy did not come back at distance 0 at its start: nothing timed' % shape)
        del key
        mem_s, mem_w = peak_above_resident(shift), peak_above_resident(windows)
        s_ms, w_ms = timed([shift, windows], args.warmup, args.runs)
        opsn = 2.0 * K * M * n * D
        rate = opsn / (s_ms[0] * 1e-3)
        rows.append({'strips': M, 'columns': T, 'C': C, 'S': S, 'K': K, 'seg': seg, 'starts': M * n, 'level_bytes': level.nbytes,
                     'window_bytes': M * n * D, 'shift_ms': s_ms, 'windows_ms': w_ms, 'ratio': w_ms[0] / s_ms[0], 'int8_ops': opsn,
                     'int8_ops_per_s': rate, 'share_of_int8_peak': rate / INT8_PEAK, 'shift_peak_bytes': mem_s, 'windows_peak_bytes': mem_w,
                     'chunk_starts': step})
        print('%-26s %4d %12.2f %12.2f %7.2f %10.1f %8.1f %12.1f %12.1f   (min/max shift %.2f/%.2f, windows %.2f/%.2f)'
              % ('%d x %d x %d x %d^2' % (M, T, C, S), K, s_ms[0], w_ms[0], w_ms[0] / s_ms[0], rate / 1e12, 100 * rate / INT8_PEAK,
                 mem_s / 2 ** 20, mem_w / 2 ** 20, s_ms[1], s_ms[2], w_ms[1], w_ms[2]), flush=True)
        del level, queries
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'runs': args.runs, 'warmup': args.warmup, 'chunk_mb': args.chunk_mb,
                       'int8_peak_ops_per_s': INT8_PEAK, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
