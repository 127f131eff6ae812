#!/usr/bin/env python
"""Cost and loss of the mel-frequency sound representation 'melif' (docs/experiments_melif.md), two measurements:

    python tools/melif_timing.py [--cases 256,256 256,1024 1024,1024] [--samples 6] [--hop 128] [--warmup 3] [--runs 7] [--inner 20]
                                 [--json out.json]

  For each (M rows, H = n_fft/2 bins), ``--samples`` test signals of hop (M - 1) + 5 samples and as many seeded images [2, M, M], in ONE
  run and alternately, so that all see the same machine:
    analysis   'melif'  phase.mel_spectrogram_stack_u8 (pg_mel_analyse_f64 + quantiser)          M rows x M frames from n_fft
               'magif'  phase.analyse(bins=H, frames=M) + phase.magif_u8 at the SAME n_fft          H rows x M frames: the yardstick
               host     sound.melif_analyse + sound.magif_image per sample, numpy, under a wall clock (one run: it takes seconds)
    synthesis  'melif'  DeviceSoundSaver(mode='melif', n_fft=2 H).to_waveforms of [2, M, M] images       four launches, M frames
               'magif'  DeviceSoundSaver(mode='magif').to_waveforms of [2, H, H] images, the image the same n_fft needs without the
                        warp (images are square): H frames, so only M = H compares like with like
               host     SoundSaver(mode='melif').image_to_sound per sample
  The device figures are HIP events around ``--inner`` back-to-back calls divided by ``--inner``, after ``--warmup`` untimed calls, the
  median of ``--runs`` (min .. max).  The mel and the host images / waveforms are compared first; the tool stops if they differ.

    python tools/melif_timing.py --roundtrip [--rows 64 256] [--sample-rate 16000]

  Host only (numpy, no GPU): analysis -> uint8 -> synthesis of a harmonic test signal with vibrato plus a noise burst, for 'magif' at
  n_fft = 2 M and for 'melif' at M = H and H = 4 M, hop = n_fft/4; the scale-invariant spectral convergence
  min_c || c |STFT(y')| - |STFT(y)| || / || STFT(y) || over all bins and over the bins below and above 1 kHz."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def test_signal(ns, seed):
    """tests/magif_ref.signal: a chirp at half scale plus noise, clipped to [-1, 1], float32."""
    t = np.arange(ns)
    y = 0.5 * np.sin(2 * np.pi * (0.01 * t + 0.2 * t * t / (2.0 * ns))) + 0.1 * np.random.RandomState(seed).randn(ns)
    return np.clip(y, -1, 1).astype(np.float32)


def harmonic_signal(ns, sr, seed=0):
    """Ten harmonics of 220 Hz with amplitudes 1/h and a 5 Hz vibrato of +-1 %, peak 0.5, plus a burst of white noise of 50 ms in the
    middle; float32."""
    t = np.arange(ns) / float(sr)
    phase = 2 * np.pi * 220.0 * (t - 0.01 / (2 * np.pi * 5.0) * np.cos(2 * np.pi * 5.0 * t))
    y = sum(np.sin(h * phase) / h for h in range(1, 11))
    y = 0.5 * y / np.abs(y).max()
    a, n = ns // 2, int(0.05 * sr)
    y[a:a + n] += 0.2 * np.random.RandomState(seed).randn(n)
    return np.clip(y, -1, 1).astype(np.float32)


def convergence(y, x, n_fft, hop, sr, sound):
    """Scale-invariant spectral convergence of x against y on the common STFT grid: over all bins, below 1 kHz, from 1 kHz up."""
    n = min(len(y), len(x))
    A, B = np.abs(sound.stft(y[:n], n_fft, hop)), np.abs(sound.stft(x[:n], n_fft, hop))
    f = np.arange(A.shape[0]) * sr / float(n_fft)
    out = []
    for sel in (slice(None), f < 1000.0, f >= 1000.0):
        a, b = A[sel], B[sel]
        c = float((a * b).sum() / (b * b).sum())
        out.append(float(np.linalg.norm(c * b - a) / np.linalg.norm(a)))
    return out


def roundtrip(args):
    import pggan_amd as pg
    sound, phase = pg.sound, pg.phase
    sr = args.sample_rate
    print('round trip analysis -> uint8 -> synthesis on the host, sample rate %d, hop n_fft/4; spectral convergence all / < 1 kHz / >= 1 kHz' % sr)
    rows = []
    for M in args.rows:
        for mode, n_fft in (('magif', 2 * M), ('melif', 2 * M), ('melif', 8 * M)):
            if n_fft > phase.MAX_N:
                continue
            hop = n_fft // 4
            y = harmonic_signal(hop * (M - 1) + n_fft, sr)
            rng = sound._mag_range(None, n_fft)
            if mode == 'magif':
                lm, fr = sound.magif_analyse(y, n_fft, hop)
                u8 = sound.magif_image(lm[:M, :M], fr[:M, :M], rng)
                spec = sound.magif_spectrum((u8.astype(np.float64) / 127.5 - 1).astype(np.float32), (-1, 1), rng)
            else:
                table = phase.mel_table(n_fft, M, sr)
                lm, fr = sound.melif_analyse(y, n_fft, hop, table)
                u8 = sound.magif_image(lm[:, :M], fr[:, :M], rng)
                spec = sound.melif_spectrum((u8.astype(np.float64) / 127.5 - 1).astype(np.float32), table, (-1, 1), rng)
            x = sound.istft(spec, hop)
            sc = convergence(y.astype(np.float64), x, 2 * M, M // 2, sr, sound)       # one grid for the three: the 'magif' transform's
            rows.append({'rows': M, 'mode': mode, 'n_fft': n_fft, 'hop': hop, 'samples': len(x), 'sc_all': sc[0], 'sc_below_1k': sc[1], 'sc_from_1k': sc[2]})
            print('M %4d  %-5s n_fft %5d hop %4d  %7d samples   %.3f   %.3f   %.3f' % (M, mode, n_fft, hop, len(x), sc[0], sc[1], sc[2]))
    return rows


def timing(args):
    import torch
    import pggan_amd as pg
    phase, sound = pg.phase, pg.sound
    pg.ops.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())

    def device_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.inner

    def host_ms(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3
    print('%s, torch %s; %d samples, hop %d, %d calls per window, median of %d' % (torch.cuda.get_device_name(dev), torch.__version__, args.samples,
                                                                                  args.hop, args.inner, args.runs))
    rows = []
    for case in args.cases:
        M, H = (int(v) for v in case.split(','))
        n_fft, hop, n = 2 * H, args.hop, args.samples
        table = phase.mel_table(n_fft, M)
        rng = phase.default_mag_range(n_fft)
        y = np.stack([test_signal(hop * (M - 1) + 5 + H, 10 + b) for b in range(n)])
        y_d = torch.from_numpy(y).to(dev)
        out = (np.random.RandomState(M + H).rand(n, 2, M, M) * 2 - 1).astype(np.float32)
        out_d = torch.from_numpy(out).to(dev)
        wide = torch.from_numpy((np.random.RandomState(H).rand(n, 2, H, H) * 2 - 1).astype(np.float32)).to(dev)
        kw = dict(create_subdirs=False, hop_length=hop)
        mel_d = pg.DeviceSoundSaver(mode='melif', n_fft=n_fft, resolution=M, **kw)
        mel_h = pg.SoundSaver(mode='melif', n_fft=n_fft, resolution=M, **kw)
        mag_d = pg.DeviceSoundSaver(mode='magif', resolution=H, **kw)
        fns = {'analysis_melif': lambda: phase.mel_spectrogram_stack_u8(y_d, n_fft, hop, table),
               'analysis_magif': lambda: phase.magif_u8(*phase.analyse(y_d, n_fft, hop, H, M), mag_range=rng),
               'synthesis_melif': lambda: mel_d.to_waveforms(out_d),
               'synthesis_magif': lambda: mag_d.to_waveforms(wide)}

        def analysis_host():
            return np.stack([sound.magif_image(*(p[:, :M] for p in sound.melif_analyse(s, n_fft, hop, table)), mag_range=rng) for s in y])

        def synthesis_host():
            return np.stack([mel_h.image_to_sound(img) for img in out])
        t_ah, t_sh = host_ms(lambda: analysis_host()), host_ms(lambda: synthesis_host())
        img_h, wav_h = analysis_host(), synthesis_host()
        differ = float((fns['analysis_melif']().cpu().numpy() != img_h).mean())
        diff = float(np.abs(fns['synthesis_melif']().cpu().numpy() - wav_h).max())
        if not (differ <= 1e-4 and diff < 1e-5):
            raise SystemExit('M %d H %d: device and host differ (%.2e of the pixels, waveforms by %.3e): nothing timed' % (M, H, differ, diff))
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = dict((k, []) for k in fns)
        for _ in range(args.runs):
            for k, fn in fns.items():
                t[k].append(device_ms(fn))
        row = {'rows': M, 'bins': H, 'n_fft': n_fft, 'samples': n, 'frames': M, 'hop': hop, 'pixels_differing_from_host': differ,
               'waveform_max_abs_diff_from_host': diff, 'analysis_host_ms': t_ah, 'synthesis_host_ms': t_sh}
        for k, v in t.items():
            row[k + '_ms'], row[k + '_ms_min_max'] = statistics.median(v), [min(v), max(v)]
        rows.append(row)
        print('M %4d H %4d  analysis: melif %.3f ms (%.3f .. %.3f), magif at n_fft %d %.3f ms (%.3f .. %.3f), host %.0f ms'
              % (M, H, row['analysis_melif_ms'], min(t['analysis_melif']), max(t['analysis_melif']), n_fft, row['analysis_magif_ms'],
                 min(t['analysis_magif']), max(t['analysis_magif']), t_ah))
        print('               synthesis: melif %.3f ms (%.3f .. %.3f), magif at %d^2 %.3f ms (%.3f .. %.3f), host %.0f ms'
              % (row['synthesis_melif_ms'], min(t['synthesis_melif']), max(t['synthesis_melif']), H, row['synthesis_magif_ms'],
                 min(t['synthesis_magif']), max(t['synthesis_magif']), t_sh))
    return {'device': torch.cuda.get_device_name(dev), 'runs': args.runs, 'warmup': args.warmup, 'inner': args.inner, 'rows': rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--roundtrip', action='store_true')
    ap.add_argument('--rows', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--sample-rate', type=int, default=16000)
    ap.add_argument('--cases', nargs='+', default=['256,256', '256,1024', '1024,1024'])
    ap.add_argument('--samples', type=int, default=6)
    ap.add_argument('--hop', type=int, default=128)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    result = {'roundtrip': roundtrip(args)} if args.roundtrip else timing(args)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
