"""Mel-frequency magnitude + instantaneous frequency ('melif') on the host: the properties of the table, the
numpy twin of sound.py against tests/melif_ref.py and, through the identity table, against the 'magif' twin; ``phase.MelTable``'s
checks, the binding table of include/pggan_hip_mel.h, the argument errors of the public functions and ``SoundSaver(mode='melif')``.
No GPU.

"The test signal" is ``magif_ref.signal`` (tests/test_magif_host.py).  Bounds: the twin and the reference are two fp64 restatements of
one formula on the SAME table (the reference's, handed to ``phase.MelTable``) and on two STFTs (batched rFFT / per-frame rFFT):
1e-12 x max|reference|, the mel IF compared on the circle and weighed with |z_m| (it is only as well defined as its row is loud), as
tests/test_magif_host.py weighs a bin's.  The two TABLES differ by the roundings of log1p / expm1 in numpy and in math: a few ulp of
the largest position, bounded below.  Every comparison prints its measured maximum before it asserts (docs/experiments_melif.md)."""
import ctypes
import os
import re

import numpy as np
import pytest

import melif_ref as ref
import pggan_amd as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = 1e-12
ULP = 2.0 ** -52


def product_table(tab):
    """The reference's table as a phase.MelTable."""
    return pg.MelTable(tab.n_fft, *tab.arrays())


# ---------------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('M,H,sr', ref.TABLES)
def test_table_properties(M, H, sr):
    n_fft = 2 * H
    t = pg.mel_table(n_fft, M, sr)
    p, q = pg.phase.mel_positions(n_fft, M, sr)
    assert (t.n_fft, t.rows, t.bins) == (n_fft, M, H) and pg.mel_table(n_fft, M, sr) is t             # built once
    sums = np.array([t.row_weights(m).sum() for m in range(M)])
    print('table M=%d H=%d sr=%d: widest band %d bins, |row sum - 1| <= %.2e' % (M, H, sr, t.count.max(), np.abs(sums - 1).max()))
    assert np.abs(sums - 1).max() <= 4 * ULP
    assert t.count.min() >= 1 and t.start.min() >= 0 and (t.start + t.count).max() <= H and (t.weights > 0).all()
    assert t.weights.shape == (int(t.count.sum()),) and np.array_equal(t.offset, np.cumsum(t.count) - t.count)
    assert (np.diff(p) > 0).all() and (np.diff(q) > 0).all()
    assert p[0] == 0.0 and p[-1] == H - 1 and q[0] == 0.0 and q[-1] == M - 1
    assert t.lower.min() >= 0 and t.lower.max() <= M - 2 and t.frac.min() >= 0.0 and t.frac.max() <= 1.0
    assert (t.lower[0], t.frac[0], t.lower[-1], t.frac[-1]) == (0, 0.0, M - 2, 1.0)
    assert np.array_equal(t.lower + t.frac, q) or np.abs(t.lower + t.frac - q).max() <= ULP * M
    # a row is a weighted MEAN: it never exceeds the loudest bin, so default_mag_range(n_fft) holds for the mel image too
    y = ref.signal(3 * n_fft, M + H)
    a, _, _, _ = ref.analyse(y, n_fft, n_fft // 2, ref.table(n_fft, M, sr))
    S = np.abs(pg.sound.stft(y, n_fft, n_fft // 2))[:H]
    b = np.stack([np.sum(t.row_weights(m)[:, None] * S[t.start[m]:t.start[m] + t.count[m]], axis=0) for m in range(M)])
    print('table M=%d H=%d: max a_m %.6f (reference %.6f) of max|S_k| %.6f' % (M, H, b.max(), a.max(), S.max()))
    assert b.max() <= S.max() and a.max() <= S.max()
    # ... and it is the reference's table up to the roundings of log1p / expm1: the same bands, positions within 8 ulp of the largest
    r = ref.table(n_fft, M, sr)
    start, count, weights, lower, frac = r.arrays()
    assert np.array_equal(start, t.start) and np.array_equal(count, t.count) and np.array_equal(lower, t.lower)
    print('table M=%d H=%d: |dp| %.2e |dq| %.2e |dW| %.2e |dfrac| %.2e' % (M, H, np.abs(p - r.p).max(), np.abs(q - r.q).max(),
                                                                       np.abs(weights - t.weights).max(), np.abs(frac - t.frac).max()))
    assert np.abs(p - r.p).max() <= 8 * ULP * H and np.abs(q - r.q).max() <= 8 * ULP * M
    assert np.abs(frac - t.frac).max() <= 8 * ULP * M and np.abs(weights - t.weights).max() <= 32 * ULP * H   # (a half-width is >= 1 bin)


def test_low_rows_interpolate_and_high_rows_average():
    """The floor of one bin: where the rows are closer than the bins (the low end of M = H) a row is the linear interpolation of its
    two neighbouring bins; where they are wider it is a triangle over its band, up to 43 bins at 128 rows of 1024."""
    t = pg.mel_table(2048, 1024)
    p, _ = pg.phase.mel_positions(2048, 1024, 16000)
    for m in (1, 2, 3, 10):
        assert p[m] - p[m - 1] < 1 and t.count[m] == 2 and t.start[m] == int(np.floor(p[m]))
        f = p[m] - np.floor(p[m])
        assert np.abs(t.row_weights(m) - [1 - f, f]).max() <= 4 * ULP
    assert t.count[0] == 1 and t.start[0] == 0 and t.count[-1] >= 2 and t.start[-1] + t.count[-1] == 1024
    assert pg.mel_table(2048, 128).count.max() == 43


# ------------------------------------------------------------------------------------------------------------ twin and reference
@pytest.mark.parametrize('n_fft,M,hop,sr', [(16, 4, 3, 16000), (64, 8, 16, 16000), (64, 32, 16, 16000), (256, 32, 64, 44100), (512, 256, 128, 16000)])
def test_host_twin_equals_the_reference(n_fft, M, hop, sr):
    r = ref.table(n_fft, M, sr)
    t = product_table(r)
    y = ref.signal(hop * (M + 2) + 5, n_fft + M)                           # M frames for the image and a ragged rest
    a, logmag, g, z = ref.analyse(y, n_fft, hop, r)
    lm, fr = pg.sound.melif_analyse(y, n_fft, hop, t)
    scale = float(np.abs(z).max())
    dist = np.abs(ref.wrap(fr - g)) * np.abs(z)
    print('host analysis n_fft=%d M=%d: |dlogmag| %.3e of max|logmag| %.3e, IF circular distance x |z| %.3e of max|z| %.3e'
          % (n_fft, M, np.abs(lm - logmag).max(), np.abs(logmag).max(), dist.max(), scale))
    assert lm.shape == fr.shape == logmag.shape == (M, 1 + len(y) // hop)
    assert np.abs(lm - logmag).max() <= TWIN * np.abs(logmag).max() and dist.max() <= TWIN * scale
    # images: no pixel differs
    mine = pg.sound.magif_image(lm[:, :M], fr[:, :M], ref.default_mag_range(n_fft))
    want, _ = ref.image(y, n_fft, hop, r)
    print('host image n_fft=%d M=%d: %d of %d pixels differ' % (n_fft, M, int((mine != want).sum()), want.size))
    assert mine.shape == want.shape == (2, M, M) and np.array_equal(mine, want)
    # synthesis, with an image that reaches the clamp and |IF| > 1
    img = ((np.random.RandomState(n_fft + M).rand(2, M, M) * 2 - 1) * 1.25).astype(np.float32)
    spec_ref, _ = ref.spectrum(img, r)
    spec = pg.sound.melif_spectrum(img, t, (-1, 1), ref.default_mag_range(n_fft))
    err = float(np.abs(spec - spec_ref).max())
    print('host spectrum n_fft=%d M=%d: max|diff| %.3e of %.3e' % (n_fft, M, err, np.abs(spec_ref).max()))
    assert spec.shape == spec_ref.shape == (n_fft // 2 + 1, M) and not spec[-1].any() and (spec_ref == 0).sum() > M
    # (the running sum of W values carries (W - 1) roundings whose order differs between a cumsum and itself only by the compiler's;
    #  what differs is cos / sin of pi c at |c| <= 1: a few ulp of the magnitude)
    assert err <= TWIN * np.abs(spec_ref).max()


@pytest.mark.parametrize('n_fft,hop', [(8, 2), (64, 16), (256, 100)])
def test_identity_table_gives_the_magif_twin_exactly(n_fft, hop):
    """One-bin rows copy their bin, frac 0 (and the last bin's frac 1) copy their row: not a single bit differs."""
    H = n_fft // 2
    t = pg.MelTable.identity(n_fft)
    assert (t.rows, t.bins) == (H, H) and t.count.tolist() == [1] * H and t.frac.tolist() == [0.0] * (H - 1) + [1.0]
    y = ref.signal(20 * n_fft, 5)
    lm, fr = pg.sound.melif_analyse(y, n_fft, hop, t)
    lm0, fr0 = pg.sound.magif_analyse(y, n_fft, hop)
    assert np.array_equal(lm, lm0[:H]) and np.array_equal(fr, fr0[:H])
    img = ((np.random.RandomState(n_fft).rand(2, H, H) * 2 - 1) * 1.5).astype(np.float32)
    assert np.array_equal(pg.sound.melif_spectrum(img, t, (-1, 1), (0.0, 3.0)), pg.sound.magif_spectrum(img, (-1, 1), (0.0, 3.0)))
    # the reference says the same of itself
    r = ref.identity(n_fft)
    s0 = ref.mref.spectrum(img, mag_range=(0.0, 3.0))
    assert np.array_equal(ref.spectrum(img, r, mag_range=(0.0, 3.0))[0], s0)
    assert np.array_equal(ref.analyse(y, n_fft, hop, r)[1], ref.mref.analyse(y, n_fft, hop)[1][:H])


def test_a_row_beside_frac_zero_bins_is_not_read():
    """frac == 0 reads row i alone: a NaN in row i + 1 does not leak into such a bin (0 x NaN would)."""
    t = pg.MelTable(16, [0, 2, 4, 6], [2, 2, 2, 2], np.full(8, 0.5), [0, 0, 1, 1, 2, 2, 2, 2], [0, 0, 0.25, 0.5, 0, 0.5, 0.75, 1])
    img = (np.random.RandomState(3).rand(2, 4, 4) * 2 - 1).astype(np.float32)
    clean = pg.sound.melif_spectrum(img, t, (-1, 1), (0.0, 2.0))
    img[:, 1, 2] = np.nan                                                  # row 1 neighbours bins 0 and 1 (frac 0) and carries bins 2 and 3
    spec = pg.sound.melif_spectrum(img, t, (-1, 1), (0.0, 2.0))
    assert np.array_equal(spec[[0, 1, 4, 5, 6, 7, 8]], clean[[0, 1, 4, 5, 6, 7, 8]])
    assert np.isnan(spec[2:4, 2:]).all() and np.array_equal(spec[2:4, :2], clean[2:4, :2])


# ------------------------------------------------------------------------------------------------------------------- MelTable
def test_mel_table_rejects_malformed_arrays():
    good = dict(start=[0, 1, 2, 2], count=[1, 2, 2, 2], weights=[1, .5, .5, .5, .5, .25, .75], lower=[0, 1, 2, 2], frac=[0, 0, 0, 1])
    t = pg.MelTable(8, **good)
    assert (t.rows, t.bins, t.n_fft) == (4, 4, 8) and t.offset.tolist() == [0, 1, 3, 5] and t.row_weights(3).tolist() == [.25, .75]
    assert t.start.dtype == t.count.dtype == t.offset.dtype == t.lower.dtype == np.int32 and t.weights.dtype == t.frac.dtype == np.float64
    with pytest.raises(ValueError):
        t.weights[0] = 2.0                                                 # read-only: a table is validated once
    bad = [dict(start=[0, 1, 2, 3], count=[1, 2, 2, 2]),                  # a band past the last bin
           dict(start=[-1, 1, 2, 2]),
           dict(count=[1, 0, 2, 2], weights=[1, .5, .5, .5, .5]),         # an empty row
           dict(count=[1, 2, 2]),                                         # lengths
           dict(weights=[1, .5, .5, .5, .5, .25]),
           dict(weights=[1, .5, .5, .5, .5, .25, float('nan')]),
           dict(weights=[1, .5, .5, .5, .5, .25, float('inf')]),
           dict(lower=[0, 1, 2, 3]),                                      # row lower + 1 does not exist
           dict(lower=[-1, 1, 2, 2]),
           dict(lower=[0, 1, 2]),
           dict(lower=[0.0, 1.0, 2.0, 2.0]),                              # not integers
           dict(frac=[0, 0, 0, 1.5]),
           dict(frac=[0, -0.1, 0, 1]),
           dict(frac=[0, float('nan'), 0, 1]),
           dict(frac=[0, 0, 1]),
           dict(start=[[0, 1], [2, 2]]),
           dict(start=[0], count=[1], weights=[1.0])]                     # one row: no pair of rows to lie between
    for change in bad:
        with pytest.raises(ValueError, match='MelTable'):
            pg.MelTable(8, **dict(good, **change))
    for n_fft in (4, 12, 4096, 8.5):
        with pytest.raises(ValueError, match='n_fft'):
            pg.MelTable(n_fft, **good)
    with pytest.raises(ValueError, match='MelTable'):
        pg.MelTable(8, **dict(good, start=[0, 0, 0, 0, 0], count=[1] * 5, weights=[1] * 5))       # more rows than bins
    for rows in (2, 3, 6, 64, 4.5, True):
        with pytest.raises(ValueError, match='rows'):
            pg.mel_table(64, rows)
    for sr in (0, -16000, float('nan'), float('inf'), 'fast', None, True):
        with pytest.raises(ValueError, match='sample_rate'):
            pg.mel_table(64, 8, sr)
    assert pg.mel_table(64, 8) is pg.mel_table(64, 8, 16000) is pg.mel_table(64, 8, 16000.0)


def test_mel_header_parses_completely():
    """Every prototype of include/pggan_hip_mel.h lands in _lib.MEL_SIGNATURES, disjoint from every other table; the product header's
    and the phase header's tables are as they were; the built library exports both names."""
    _lib = pg._lib
    with open(os.path.join(ROOT, 'include', 'pggan_hip_mel.h')) as f:
        text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', f.read(), flags=re.S)
    protos = re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', text)
    assert sorted(protos) == sorted(_lib.MEL_SIGNATURES) == ['pg_mel_analyse_f64', 'pg_mel_spectrum_f64']
    defines = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(PG_\w+)[ \t]+(\S+)[ \t]*$', text, flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == _lib.MEL_CONSTANTS == {}         # the limits are pggan_hip_phase.h's
    P, I, L, D = _lib.P, _lib.I, _lib.L, _lib.D
    assert _lib.MEL_SIGNATURES['pg_mel_analyse_f64'] == [P, L, I, P, P, I, I, I, I, P, P, P, P, P]
    assert _lib.MEL_SIGNATURES['pg_mel_spectrum_f64'] == [P, P, P, I, I, I, I, P, P, D, D, D, D, D, D, P]
    others = (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.CLUSTER_SIGNATURES, _lib.GAN_SIGNATURES, _lib.PHASE_SIGNATURES,
              _lib.SAMPLING_SIGNATURES, _lib.PROJECTION_SIGNATURES, _lib.CROP_SIGNATURES, _lib.SWD_SIGNATURES)
    assert not any(set(_lib.MEL_SIGNATURES) & set(o) for o in others)
    assert len(_lib.SIGNATURES) == 96 and len(_lib.CONSTANTS) == 27 and _lib.ABI_VERSION == 27 and len(_lib.PHASE_SIGNATURES) == 5
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    for name in protos:
        assert hasattr(lib, name), name
    fns = pg._lib.load()
    for name in protos:
        fn = getattr(fns, name)
        assert list(fn.argtypes) == _lib.MEL_SIGNATURES[name] and fn.restype is _lib.I, name
    assert {'MelTable', 'mel_table', 'mel_analyse', 'mel_spectrum', 'mel_synthesise'} <= set(pg.__all__)
    assert pg.MelTable is pg.phase.MelTable and pg.mel_table is pg.phase.mel_table


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_arguments():
    import torch
    y = ref.signal(600, 1)
    # sample_rate / mel_rows belong to 'melif', n_fft (of a saver) too; unknown modes keep their error
    for kw in (dict(mel_rows=8), dict(sample_rate=16000)):
        for mode in ('abslog', 'magif', 'raw'):
            with pytest.raises(ValueError, match='melif'):
                pg.spectrogram_u8(y, 64, 16, img_mode=mode, **kw)
        with pytest.raises(ValueError, match='melif'):
            pg.spectrogram_stack_u8(y[None], 64, 16, **kw)
        with pytest.raises(ValueError, match='melif'):
            pg.spectrogram_strip_u8(y, 64, 16, **kw)
        with pytest.raises(ValueError, match='melif'):
            pg.spectrogram_strip_u8(y, 64, 16, img_mode='abslog', **kw)
        with pytest.raises(ValueError, match='melif'):
            pg.DeviceStripDataset.from_waveforms([y], 64, 16, **kw)
    with pytest.raises(ValueError, match='img_mode'):
        pg.spectrogram_u8(y, 64, 16, img_mode='ifmel')
    with pytest.raises(ValueError, match='img_mode'):
        pg.spectrogram_u8(y, 64, 16, img_mode='ifmel', mel_rows=8)
    with pytest.raises(ValueError, match='img_mode'):
        pg.spectrogram_stack_u8(y[None], 64, 16, img_mode='abslog')
    with pytest.raises(ValueError, match='img_mode'):
        pg.spectrogram_strip_u8(y, 64, 16, img_mode='reallog')
    for mode in ('abslog', 'reallog', 'raw', 'magif'):
        with pytest.raises(ValueError, match='n_fft'):
            pg.SoundSaver(create_subdirs=False, mode=mode, n_fft=64)
        with pytest.raises(ValueError, match='n_fft'):
            pg.DeviceSoundSaver(create_subdirs=False, mode=mode, n_fft=64)
    with pytest.raises(ValueError, match='n_fft'):
        pg.SoundSaver(create_subdirs=False, mode='melif', n_fft=64.5)
    with pytest.raises(ValueError, match='mag_range'):
        pg.SoundSaver(create_subdirs=False, mode='melif', mag_range=(1.0, 1.0))
    assert pg.SoundSaver(create_subdirs=False, mode='melif', mag_range=(0, 2)).mag_range == (0.0, 2.0)
    # the table's arguments are checked before anything is uploaded (no GPU here)
    for kw, what in ((dict(mel_rows=64), 'rows'), (dict(mel_rows=6), 'rows'), (dict(sample_rate=0), 'sample_rate')):
        with pytest.raises(ValueError, match=what):
            pg.spectrogram_u8(y, 64, 16, img_mode='melif', **kw)
        with pytest.raises(ValueError, match=what):
            pg.spectrogram_stack_u8(y[None], 64, 16, img_mode='melif', **kw)
        with pytest.raises(ValueError, match=what):
            pg.spectrogram_strip_u8(y, 64, 16, img_mode='melif', **kw)
    with pytest.raises(ValueError, match='n_fft'):
        pg.spectrogram_u8(y, 48, 16, img_mode='melif')
    for kw in (dict(mel_rows=8), dict(sample_rate=16000)):                  # the misplaced argument is named, not the frame count of a short waveform
        with pytest.raises(ValueError, match='melif'):
            pg.DeviceStripDataset.from_waveforms([y[:100]], 64, 16, **kw)
    with pytest.raises(ValueError, match='rows'):
        pg.DeviceStripDataset.from_waveforms([y[:100]], 64, 16, 'melif', mel_rows=64)
    with pytest.raises(ValueError, match='waveform 0'):                     # 600 samples every 16: 37 usable frames, the window needs 32 / 64
        pg.DeviceStripDataset.from_waveforms([y], 128, 16, 'melif', mel_rows=64)
    with pytest.raises(ValueError, match='two-channel'):
        pg.SoundSaver(create_subdirs=False, mode='melif').image_to_sound(np.zeros((16, 16), np.float32))
    with pytest.raises(ValueError, match='rows'):                           # n_fft/2 = 8 bins cannot carry 16 rows
        pg.SoundSaver(create_subdirs=False, mode='melif', n_fft=16).image_to_sound(np.zeros((2, 16, 16), np.float32))
    # host tensors never reach a kernel; a table is a MelTable, for this n_fft and these rows
    t = pg.mel_table(64, 8)
    with pytest.raises(ValueError, match='signals'):
        pg.mel_analyse(torch.zeros(2, 100), 64, 16, t)
    with pytest.raises(ValueError, match='images'):
        pg.mel_spectrum(torch.zeros(2, 2, 8, 8), t)
    with pytest.raises(ValueError, match='images'):
        pg.mel_synthesise(torch.zeros(2, 2, 8, 8, dtype=torch.float64), 8, t)
    with pytest.raises(ValueError, match='melif_analyse'):
        pg.sound.melif_analyse(y, 32, 8, t)
    with pytest.raises(ValueError, match='melif_spectrum'):
        pg.sound.melif_spectrum(np.zeros((2, 16, 16), np.float32), t, (-1, 1), (0.0, 1.0))
    assert pg.sound.strip_frames(600, 16, 'melif') == 37


# ----------------------------------------------------------------------------------------------------------------------- saver
@pytest.mark.parametrize('M,n_fft,hop,sr', [(16, None, 8, 16000), (16, 128, 32, 44100)])
def test_host_saver_equals_the_reference_and_repeats_itself(M, n_fft, hop, sr, tmp_path):
    from scipy.io import wavfile
    out = ((np.random.RandomState(M).rand(2, 2, M, M) * 2 - 1) * 1.25).astype(np.float32)
    r = ref.table(2 * M if n_fft is None else n_fft, M, sr)
    names = ['fakes_sound_000003_00.wav', 'fakes_sound_000003_01.wav']
    waves = []
    for run in ('a', 'b'):
        saver = pg.SoundSaver(str(tmp_path / run), resolution=2 * M, hop_length=hop, mode='melif', seed=5, sample_rate=sr, n_fft=n_fft)
        state = saver._rng.get_state()
        saver(out, 3)
        assert sorted(os.listdir(str(tmp_path / run))) == names
        assert all(np.array_equal(a, b) for a, b in zip(state, saver._rng.get_state()))        # no random start
        waves.append([wavfile.read(str(tmp_path / run / n)) for n in names])
    for i in range(2):
        (sr_a, a), (sr_b, b) = waves[0][i], waves[1][i]
        want = ref.synthesise(out[i], hop, r)
        got = saver.image_to_sound(out[i])
        err = float(np.abs(got - want / np.abs(want).max()).max())
        print('host saver M=%d n_fft=%s sample %d: max|diff| %.3e of a peak of 1' % (M, n_fft, i, err))
        assert sr_a == sr_b == sr and a.dtype == np.float32 and np.array_equal(a, b)             # the same WAV twice
        assert got.shape == want.shape == ((M - 1) * hop,) and err <= 1e-9                        # (tests/test_magif_host.py's bound)
        assert np.abs(a - (want / np.abs(want).max()).repeat(2)).max() < 1e-5
