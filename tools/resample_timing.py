#!/usr/bin/env python
"""Cost of the rate conversion (docs/experiments_resample.md): ``sound.resample`` on the device, its numpy twin and
``scipy.signal.resample_poly`` on the host, and ``DeviceStripDataset.from_wav_files`` end to end.

    python tools/resample_timing.py [--seconds 600] [--twin-seconds 60] [--warmup 3] [--runs 7] [--inner 5] [--files 10]
                                    [--tmp DIR] [--json out.json]

  Three workloads of ``--seconds`` of seeded noise: 44100 -> 16000 Hz stereo int16, 48000 -> 16000 Hz mono float32 and
  16000 -> 44100 Hz mono float32.  For each:
    device   sound.resample on a signal that is already in HBM (one launch of pg_resample_mono and the allocation of its output): HIP
             events around ``--inner`` back-to-back calls divided by ``--inner``, after ``--warmup`` untimed calls, the median of
             ``--runs`` (min .. max); input bytes per second = the bytes of the signal over that time
    twin     sound.resample(device='cpu'), one run under a wall clock on the first ``--twin-seconds`` seconds (it loops over the taps in
             Python), first held against the device result of the same piece: the tool stops if a bit differs
    scipy    mix-down in float32 + scipy.signal.resample_poly(m, L, M, window=('kaiser', beta)) on the whole signal, wall clock, median
             of 3 -- another filter (scipy designs its own Kaiser FIR), the yardstick for what the host path costs
  End to end, ``--files`` WAV files of the first workload written to ``--tmp``:
    device   DeviceStripDataset.from_wav_files(paths, frequency=16000), wall clock to a device synchronise
    host     load_wav + mix-down + resample_poly per file, then DeviceStripDataset.from_waveforms, the same way
  each once after a warm-up with one file, alternately, twice."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

WORKLOADS = [('44100 -> 16000, stereo int16', 44100, 16000, 2, np.int16),
             ('48000 -> 16000, mono float32', 48000, 16000, 1, np.float32),
             ('16000 -> 44100, mono float32', 16000, 44100, 1, np.float32)]


def noise(nsamp, channels, dtype, seed):
    rs = np.random.RandomState(seed)
    shape = (nsamp,) if channels == 1 else (nsamp, channels)
    if dtype == np.int16:
        return rs.randint(-16384, 16384, size=shape).astype(np.int16)
    return (rs.rand(*shape) - 0.5).astype(np.float32)


def med(values):
    return '%.3f (%.3f .. %.3f)' % (statistics.median(values), min(values), max(values))


def host_resample(x, L, M, beta):
    from scipy.signal import resample_poly
    m = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x
    if m.ndim == 2:
        m = m.sum(axis=1) / np.float32(2)
    return resample_poly(m, L, M, window=('kaiser', beta)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=int, default=600)
    ap.add_argument('--twin-seconds', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--files', type=int, default=10)
    ap.add_argument('--tmp', default=None)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import torch
    import pggan_amd as pg
    from scipy.io import wavfile
    sound = pg.sound
    if not torch.cuda.is_available():
        raise SystemExit('resample_timing: needs a GPU (there is no fallback)')
    results = {'seconds': args.seconds, 'twin_seconds': args.twin_seconds, 'workloads': []}
    for name, rate_in, rate_out, channels, dtype in WORKLOADS:
        x = noise(args.seconds * rate_in, channels, dtype, 1)
        table = sound.resample_table(rate_in, rate_out)
        x_d = torch.from_numpy(x).cuda()
        table.on(x_d.device)
        # the twin on the first piece, and the device against it
        piece = x[:args.twin_seconds * rate_in]
        t0 = time.perf_counter()
        twin = sound.resample(piece, rate_in, rate_out, device='cpu')
        twin_s = time.perf_counter() - t0
        got = sound.resample(piece, rate_in, rate_out).cpu().numpy()
        if not np.array_equal(got, twin):
            raise SystemExit('%s: the device and the twin differ in %d of %d outputs' % (name, int((got != twin).sum()), twin.size))
        for _ in range(args.warmup):
            out = sound.resample(x_d, rate_in, rate_out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                out = sound.resample(x_d, rate_in, rate_out)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.inner)
        sci = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = host_resample(x, table.L, table.M, sound.RESAMPLE_BETA)
            sci.append(time.perf_counter() - t0)
        body = slice(1000, -1000)
        dev = float(np.abs(out.cpu().numpy()[body] - ref[body]).max())
        row = dict(name=name, L=table.L, M=table.M, T=table.T, n_in=int(x.shape[0]), n_out=int(out.shape[0]), input_bytes=int(x.nbytes),
                   device_ms=ms, twin_s=twin_s, scipy_s=sci, max_abs_diff_to_scipy=dev)
        results['workloads'].append(row)
        print('%s (L %d, M %d, T %d; %d -> %d samples, %.1f MB in)' % (name, table.L, table.M, table.T, x.shape[0], out.shape[0], x.nbytes / 1e6))
        print('  device  %s ms per call, %.1f GB/s of input' % (med(ms), x.nbytes / statistics.median(ms) / 1e6))
        print('  twin    %.2f s for the first %d s of the signal (equal to the device bit for bit)' % (twin_s, args.twin_seconds))
        print('  scipy   %s s (resample_poly; max |device - scipy| away from the ends %.2e)' % (med(sci), dev), flush=True)
        del x_d, out
    # ---------------------------------------------------------------------------------------------------- end to end
    name, rate_in, rate_out, channels, dtype = WORKLOADS[0]
    L, M = sound._ratio(rate_in, rate_out)
    tmp = args.tmp or tempfile.mkdtemp(prefix='resample_timing_')
    paths = []
    for i in range(args.files):
        paths.append(os.path.join(tmp, 'file%02d.wav' % i))
        wavfile.write(paths[-1], rate_in, noise(args.seconds * rate_in, channels, dtype, 10 + i))
    kw = dict(n_fft=1024, hop_length=128)

    def device_path(ps):
        ds = pg.DeviceStripDataset.from_wav_files(ps, frequency=rate_out, **kw)
        torch.cuda.synchronize()
        return ds

    def host_path(ps):
        ys = [host_resample(sound.load_wav(p)[1], L, M, sound.RESAMPLE_BETA) for p in ps]
        ds = pg.DeviceStripDataset.from_waveforms(ys, **kw)
        torch.cuda.synchronize()
        return ds

    device_path(paths[:1]), host_path(paths[:1])
    e2e = {'device': [], 'host': []}
    for _ in range(2):
        for key, fn in (('device', device_path), ('host', host_path)):
            t0 = time.perf_counter()
            ds = fn(paths)
            e2e[key].append(time.perf_counter() - t0)
            lengths = ds.lengths
            del ds
            torch.cuda.empty_cache()
    for p in paths:
        os.remove(p)
    results['end_to_end'] = dict(files=args.files, seconds_each=args.seconds, lengths=lengths, **e2e)
    print('end to end, %d files of %d s (%s), n_fft 1024, hop 128, %d columns each:' % (args.files, args.seconds, name, lengths[0]))
    print('  from_wav_files (device resampling)           %s s' % ', '.join('%.2f' % v for v in e2e['device']))
    print('  load_wav + resample_poly + from_waveforms    %s s' % ', '.join('%.2f' % v for v in e2e['host']))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
