#!/usr/bin/env python
"""Did a change under csrc/phase.hip change a bit of what the 'magif' entry points compute (docs/experiments_melif.md)?

    python tools/phase_bits.py --json new.json                 in this checkout, on a GPU
    python tools/phase_bits.py --json old.json                 a copy of this file in a built checkout of the other commit
    python tools/phase_bits.py --compare old.json new.json     no GPU needed; exit status 1 if any output differs

Hashes (SHA-256 of the bytes) of the outputs of ``phase.analyse`` (bins n_fft/2 and n_fft/2 + 1), ``phase.spectrogram_stack_u8``,
``phase.spectrum`` (with and without the phase output) and ``phase.synthesise`` on seeded inputs: the shapes of tests/test_magif_gpu.py
and a few beside them, 41 outputs.  The kernels are deterministic, so equal hashes from two builds mean equal bits.  Uses nothing that
an earlier checkout with phase.py lacks."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ANALYSIS = ((8, 2, 1), (8, 128, 2), (16, 3, 2), (64, 16, 3), (512, 128, 2), (2048, 128, 1), (1024, 100, 2))             # n_fft, hop, batch
SYNTHESIS = ((4, 128, 1, 1.0), (8, 3, 2, 1.0), (16, 8, 3, 1.5), (64, 128, 1, 1.0), (256, 128, 2, 1.0), (512, 64, 1, 1.25),
             (1024, 128, 1, 1.0))                                                                                          # H, hop, batch, scale


def hashes():
    import numpy as np
    import torch
    import pggan_amd as pg
    pg.ops.require_gpu()
    phase = pg.phase

    def h(t):
        return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def signal(ns, seed):                                                  # tests/magif_ref.signal
        t = np.arange(ns)
        y = 0.5 * np.sin(2 * np.pi * (0.01 * t + 0.2 * t * t / (2.0 * ns))) + 0.1 * np.random.RandomState(seed).randn(ns)
        return np.clip(y, -1, 1).astype(np.float32)
    out = {}
    for n_fft, hop, batch in ANALYSIS:
        y = torch.from_numpy(np.stack([signal(hop * (n_fft // 2 - 1) + 5, n_fft + b) for b in range(batch)])).cuda()
        for bins in (n_fft // 2, n_fft // 2 + 1):
            lm, fr = phase.analyse(y, n_fft, hop, bins)
            out['analyse n_fft %d hop %d bins %d' % (n_fft, hop, bins)] = h(lm) + h(fr)
        out['image n_fft %d' % n_fft] = h(phase.spectrogram_stack_u8(y, n_fft, hop))
    for H, hop, batch, scale in SYNTHESIS:
        img = torch.from_numpy(((np.random.RandomState(H).rand(batch, 2, H, H) * 2 - 1) * scale).astype(np.float32)).cuda()
        s, c = phase.spectrum(img, return_phase=True)
        out['spectrum H %d' % H] = h(torch.view_as_real(s)) + h(c)
        out['spectrum H %d, no phase output, mag_range (0, 2)' % H] = h(torch.view_as_real(phase.spectrum(img, mag_range=(0.0, 2.0))))
        out['synthesise H %d hop %d' % (H, hop)] = h(phase.synthesise(img, hop))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--compare', nargs=2, metavar=('OLD', 'NEW'))
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        print('%d outputs compared, %d differ%s' % (len(set(a) | set(b)), len(bad), ': ' + ', '.join(bad) if bad else ''))
        sys.exit(1 if bad else 0)
    out = hashes()
    print('%d outputs hashed' % len(out))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
