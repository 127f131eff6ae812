"""Mel-frequency magnitude + instantaneous frequency on the device (csrc/mel.hip, phase.py's ``mel_*``, sound.py's 'melif' modes, the
strip dataset) on the MI355X -- against tests/melif_ref.py (numpy fp64 on oracle/sound_steps.py), never against another kernel, except
for the IDENTITY table, which holds the fused kernels to pg_phase_analyse_f64 / pg_phase_spectrum_f64 bit for bit.

The kernel comparisons hand the product the REFERENCE's table (``MelTable(n_fft, *melif_ref.table(...).arrays())``): the kernels take
any table, and the few ulp between the two tables' positions (tests/test_melif_host.py bounds them) would otherwise be multiplied by
the 1023 steps of a running sum.  The end-to-end comparisons use the product's own ``mel_table``.

Bounds: 1e-9 x max|reference| between independent fp64 transforms (tests/test_magif_gpu.py); the mel IF is compared on the circle and
weighed with |z_m|, |wrap(got - ref)| |z_m| <= 1e-9 max|z|, and no element is excluded.  Images: a pixel may differ by one level (on
the circle for channel 1) only where the reference's value before rint lies within 1e-6 of a half-integer; such pixels are at most
1e-4 of the reference's image, every other pixel is equal.  Every comparison prints its measured maximum before it asserts
(docs/experiments_melif.md)."""
import functools
import os

import numpy as np
import pytest
import torch

import melif_ref as ref
import pggan_amd as pg

pytestmark = pytest.mark.gpu

BOUND = 1e-9
# (n_fft, M, hop, batch, sample rate)
ANALYSIS = [(8, 4, 2, 1, 16000),
            (16, 4, 3, 2, 16000),          # 2x oversampled, odd hop
            (32, 4, 8, 1, 16000),          # bands wider than M
            (64, 8, 16, 3, 16000),
            (64, 8, 16, 3, 44100),         # ... and at another sample rate
            (64, 32, 128, 2, 16000),       # hop > n_fft
            (512, 256, 128, 2, 16000),     # the largest small-LDS size
            (2048, 1024, 128, 1, 16000),   # the LDS limit; one- and two-bin rows at the low end
            (2048, 128, 128, 1, 16000)]    # the 43-bin bands
# (M, H, hop, batch, scale)
SYNTHESIS = [(4, 4, 128, 1, 1.0), (4, 8, 3, 2, 1.0), (8, 32, 8, 3, 1.0), (64, 64, 128, 1, 1.0), (256, 1024, 128, 1, 1.0),
             (1024, 1024, 128, 1, 1.0), (8, 32, 8, 2, 1.5)]       # the last one reaches the clamp and |IF| > 1


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()                # (a writable copy: the shared references stay read-only)


@functools.lru_cache(maxsize=None)
def _table(n_fft, M, sr=16000):
    """(the reference's table, the same arrays as a phase.MelTable)"""
    r = ref.table(n_fft, M, sr)
    return r, pg.MelTable(n_fft, *r.arrays())


@functools.lru_cache(maxsize=None)
def _analysis_case(n_fft, M, hop, batch, sr):
    """Signals with enough samples for M frames and a ragged rest, and the reference's a, logmag, mel IF and z per sample."""
    ns = max(hop * (M - 1) + 5, n_fft // 2 + 1)
    y = np.stack([ref.signal(ns, 100 * n_fft + hop + M + b) for b in range(batch)])
    r, _ = _table(n_fft, M, sr)
    a, logmag, g, z = (np.stack(x) for x in zip(*[ref.analyse(y[b], n_fft, hop, r) for b in range(batch)]))
    for x in (y, a, logmag, g, z):
        x.setflags(write=False)
    return y, a, logmag, g, z


@functools.lru_cache(maxsize=None)
def _synthesis_case(M, H, hop, batch, scale):
    rs = np.random.RandomState(1000 * M + H + hop)
    img = ((rs.rand(batch, 2, M, M) * 2 - 1) * scale).astype(np.float32)
    r, _ = _table(2 * H, M)
    spec, c = (np.stack(x) for x in zip(*[ref.spectrum(im, r) for im in img]))      # [batch, H + 1, W], [batch, H, W]
    for x in (img, spec, c):
        x.setflags(write=False)
    return img, spec, c


def _close(got, want, what, scale=None):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max()) if scale is None else scale
    print('%s: max|diff| %.3e, max|ref| %.3e, relative %.3e' % (what, err, scale, err / scale))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= BOUND * scale, (what, err, scale)


def _same_image(got, want, before, what):
    """The half-integer rule of the module docstring.  ``before``: the reference's values before rint, [.., 2, M, frames]."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    near = np.abs(before - np.floor(before) - 0.5) <= 1e-6
    print('%s: %d of %d reference pixels within 1e-6 of a half-integer, %d pixels differ' % (what, int(near.sum()), near.size, int((got != want).sum())))
    assert near.mean() <= 1e-4                                             # (on the reference alone; ~2e-6 of probability per pixel)
    d = np.abs(got.astype(int) - want.astype(int))
    ch = np.arange(d.shape[-3]).reshape(-1, 1, 1)
    d = np.where(ch == 1, np.minimum(d, 256 - d), d)                       # channel 1: levels on the circle
    assert np.array_equal(got[~near], want[~near]) and d.max() <= 1


# ------------------------------------------------------------------------------------------------------------------ analysis
@pytest.mark.parametrize('n_fft,M,hop,batch,sr', ANALYSIS)
def test_analysis(n_fft, M, hop, batch, sr):
    y, a, logmag, g, z = _analysis_case(n_fft, M, hop, batch, sr)
    _, t = _table(n_fft, M, sr)
    lm, fr = pg.mel_analyse(_dev(y), n_fft, hop, t)
    assert lm.dtype == fr.dtype == torch.float64 and tuple(lm.shape) == tuple(fr.shape) == logmag.shape == (batch, M, 1 + y.shape[1] // hop)
    lm, fr = lm.cpu().numpy(), fr.cpu().numpy()
    dist = np.abs(ref.wrap(fr - g)) * np.abs(z)
    print('analysis n_fft=%d M=%d hop=%d sr=%d (widest band %d): |dlogmag| %.3e of max %.3e, IF circular distance x |z| %.3e of max|z| %.3e'
          % (n_fft, M, hop, sr, t.count.max(), np.abs(lm - logmag).max(), logmag.max(), dist.max(), np.abs(z).max()))
    assert np.isfinite(lm).all() and fr.min() >= -1.0 and fr.max() <= 1.0
    assert np.abs(lm - logmag).max() <= BOUND * logmag.max() and dist.max() <= BOUND * np.abs(z).max()
    assert a.max() <= n_fft // 2 and lm.max() <= pg.phase.default_mag_range(n_fft)[1]          # the default range never clips


def test_analysis_with_cropped_frames_and_of_silence():
    n_fft, M, hop, batch, sr = ANALYSIS[3]
    y, _, logmag, g, z = _analysis_case(n_fft, M, hop, batch, sr)
    _, t = _table(n_fft, M, sr)
    F = 5                                                                  # of the 8 frames there are
    full = pg.mel_analyse(_dev(y), n_fft, hop, t)
    lm, fr = pg.mel_analyse(_dev(y), n_fft, hop, t, frames=F)
    assert tuple(lm.shape) == tuple(fr.shape) == (batch, M, F) and logmag.shape[2] > F
    assert torch.equal(lm, full[0][:, :, :F]) and torch.equal(fr, full[1][:, :, :F])           # a frame does not know how many there are
    dist = np.abs(ref.wrap(fr.cpu().numpy() - g[:, :, :F])) * np.abs(z[:, :, :F])
    print('cropped analysis: |dlogmag| %.3e, weighted IF distance %.3e' % (np.abs(lm.cpu().numpy() - logmag[:, :, :F]).max(), dist.max()))
    assert np.abs(lm.cpu().numpy() - logmag[:, :, :F]).max() <= BOUND * logmag.max() and dist.max() <= BOUND * np.abs(z).max()
    one = pg.mel_analyse(_dev(y[0]), n_fft, hop, t)                         # [nsamp]
    assert torch.equal(one[0][0], full[0][0]) and torch.equal(one[1][0], full[1][0])
    lm, fr = pg.mel_analyse(torch.zeros(2, 300).cuda(), n_fft, hop, t)      # z == 0: IF 0, not atan2(0, 0)'s choice
    assert tuple(lm.shape) == (2, M, 19) and not lm.any() and not fr.any()


@pytest.mark.parametrize('n_fft,M,hop,batch,sr', ANALYSIS)
def test_uint8_image(n_fft, M, hop, batch, sr):
    y, _, _, _, _ = _analysis_case(n_fft, M, hop, batch, sr)
    r, t = _table(n_fft, M, sr)
    want, before = (np.stack(x) for x in zip(*[ref.image(y[b], n_fft, hop, r) for b in range(batch)]))
    got = pg.phase.mel_spectrogram_stack_u8(_dev(y), n_fft, hop, t)
    assert got.is_cuda and tuple(got.shape) == (batch, 2, M, M)
    _same_image(got, want, before, 'uint8 image n_fft=%d M=%d hop=%d sr=%d' % (n_fft, M, hop, sr))


# ----------------------------------------------------------------------------------------------------------------- synthesis
@pytest.mark.parametrize('M,H,hop,batch,scale', SYNTHESIS)
def test_synthesis(M, H, hop, batch, scale):
    from oracle import sound_steps as oss
    img, spec_ref, c_ref = _synthesis_case(M, H, hop, batch, scale)
    _, t = _table(2 * H, M)
    W = M
    spec, c = pg.mel_spectrum(_dev(img), t, return_phase=True)
    assert spec.dtype == torch.complex128 and tuple(spec.shape) == (batch, W, H + 1) and tuple(c.shape) == (batch, H, W)
    if scale > 1.0:
        _, d = ref.rows_to_bins(img[0], _table(2 * H, M)[0])
        # |IF| > 1 is a phase step like any other; a bin is silent where both of its rows are clamped (the Nyquist bin is not counted)
        assert np.abs(d).max() > 1.0 and (spec_ref[0][:H] == 0).sum() > 0
    _close(c, c_ref, 'running sum M=%d H=%d' % (M, H))
    _close(spec.cpu().numpy(), spec_ref.transpose(0, 2, 1), 'spec M=%d H=%d hop=%d' % (M, H, hop))
    assert not spec[:, :, H].cpu().numpy().any()                           # the Nyquist bin
    wave_ref = np.stack([oss.istft(s, hop) for s in spec_ref])
    wave = pg.mel_synthesise(_dev(img), hop, t)
    assert tuple(wave.shape) == (batch, hop * (W - 1)) and wave.dtype == torch.float64
    _close(wave, wave_ref, 'waveform M=%d H=%d hop=%d' % (M, H, hop))
    plain = pg.mel_spectrum(_dev(img), t)                                  # without the phase output
    assert torch.equal(torch.view_as_real(plain), torch.view_as_real(spec))


def test_a_row_beside_frac_zero_bins_is_not_read():
    """frac == 0 reads row i ALONE: with a NaN in row 1, the bins 0 and 1 below it (lower 0, frac 0) keep their bits, the bins 2 and 3
    that row 1 carries are NaN from the NaN's column on, and every other bin keeps its bits."""
    t = pg.MelTable(16, [0, 2, 4, 6], [2, 2, 2, 2], np.full(8, 0.5), [0, 0, 1, 1, 2, 2, 2, 2], [0, 0, 0.25, 0.5, 0, 0.5, 0.75, 1])
    r = ref.Table(16, 4, None, t.lower.astype(np.int64), t.frac, None, None)
    img = (np.random.RandomState(3).rand(1, 2, 4, 4) * 2 - 1).astype(np.float32)
    clean, c_clean = pg.mel_spectrum(_dev(img), t, mag_range=(0.0, 2.0), return_phase=True)
    want, c_want = ref.spectrum(img[0], r, mag_range=(0.0, 2.0))
    _close(clean.cpu().numpy()[0], want.T, 'explicit table, clean image')
    img[0, :, 1, 2] = np.nan
    spec, c = pg.mel_spectrum(_dev(img), t, mag_range=(0.0, 2.0), return_phase=True)
    spec, clean = spec.cpu().numpy()[0].T, clean.cpu().numpy()[0].T        # [H + 1, W]
    keep = [0, 1, 4, 5, 6, 7, 8]
    assert np.array_equal(spec[keep], clean[keep]) and np.array_equal(c.cpu().numpy()[0][keep[:-1]], c_clean.cpu().numpy()[0][keep[:-1]])
    assert np.isnan(spec[2:4, 2:]).all() and np.array_equal(spec[2:4, :2], clean[2:4, :2])
    want, _ = ref.spectrum(img[0], r, mag_range=(0.0, 2.0))
    assert np.array_equal(np.isnan(want), np.isnan(spec))


# ------------------------------------------------------------------------------------------------------------- identity table
@pytest.mark.parametrize('H,hop,frames', [(4, 2, None), (64, 16, None), (1024, 128, 48)])
def test_identity_table_gives_the_bits_of_the_magif_kernels(H, hop, frames):
    """One-bin rows copy their bin; frac 0 (and the last bin's frac 1) read one row: mel_analyse is analyse(bins=H) and mel_spectrum is
    spectrum, bit for bit."""
    n_fft = 2 * H
    t = pg.MelTable.identity(n_fft)
    ns = max(hop * (H - 1) + 5, H + 1) if frames is None else hop * (frames - 1) + 5 + H
    y = _dev(np.stack([ref.signal(ns, 7 + b) for b in range(2)]))
    lm0, fr0 = pg.phase.analyse(y, n_fft, hop, H, frames)
    lm, fr = pg.mel_analyse(y, n_fft, hop, t, frames)
    assert tuple(lm.shape) == tuple(lm0.shape) and torch.equal(lm, lm0) and torch.equal(fr, fr0)
    img = _dev(((np.random.RandomState(H).rand(2, 2, H, H) * 2 - 1) * 1.25).astype(np.float32))
    s0, c0 = pg.phase.spectrum(img, return_phase=True)
    s, c = pg.mel_spectrum(img, t, return_phase=True)
    assert torch.equal(torch.view_as_real(s), torch.view_as_real(s0)) and torch.equal(c, c0)
    assert torch.equal(pg.mel_synthesise(img, hop, t), pg.phase.synthesise(img, hop))


def test_two_calls_give_the_same_bits():
    y = _dev(_analysis_case(*ANALYSIS[3])[0])
    _, t = _table(64, 8)
    first, second = pg.mel_analyse(y, 64, 16, t), pg.mel_analyse(y, 64, 16, t)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    big = _dev(_analysis_case(*ANALYSIS[8])[0])
    _, tb = _table(2048, 128)
    first, second = pg.mel_analyse(big, 2048, 128, tb), pg.mel_analyse(big, 2048, 128, tb)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    img = _dev(_synthesis_case(8, 32, 8, 3, 1.0)[0])
    _, ts = _table(64, 8)
    a, b = pg.mel_spectrum(img, ts, return_phase=True), pg.mel_spectrum(img, ts, return_phase=True)
    assert torch.equal(torch.view_as_real(a[0]), torch.view_as_real(b[0])) and torch.equal(a[1], b[1])
    assert torch.equal(pg.mel_synthesise(img, 8, ts), pg.mel_synthesise(img, 8, ts))


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_public_image_functions():
    """spectrogram_u8 / spectrogram_stack_u8 / spectrogram_strip_u8 with img_mode='melif' and the product's OWN table."""
    n_fft, M, hop = 64, 8, 16
    y = np.stack([ref.signal(hop * 40 + 5, 60 + b) for b in range(3)])
    for sr in (16000, 44100):
        r = ref.table(n_fft, M, sr)
        want, before = (np.stack(x) for x in zip(*[ref.image(s, n_fft, hop, r) for s in y]))
        got = pg.spectrogram_stack_u8(y.copy(), n_fft, hop, img_mode='melif', sample_rate=sr, mel_rows=M)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 2, M, M)
        _same_image(got, want, before, 'spectrogram_stack_u8 melif sr=%d' % sr)
        one = pg.spectrogram_u8(y[0].copy(), n_fft, hop, img_mode='melif', sample_rate=sr, mel_rows=M)
        assert tuple(one.shape) == (2, M, M) and torch.equal(one, got[0])
    # the defaults: 16 kHz and n_fft/2 rows; a two-column signal is mixed down first (sum / 2 in float32); an explicit range
    r = ref.table(n_fft, n_fft // 2)
    stereo = np.stack([y[0], y[2]], axis=1)
    mono = (stereo.sum(axis=1) / 2).astype(np.float32)
    want, before = ref.image(mono, n_fft, hop, r, (0.0, 3.0))
    got = pg.spectrogram_u8(stereo, n_fft, hop, img_mode='melif', mag_range=(0.0, 3.0))
    _same_image(got, want, before, 'spectrogram_u8 melif, defaults')
    # the strip: all frames but the first, [2, M, T]
    T = y.shape[1] // hop
    r = ref.table(n_fft, M)
    want, before = ref.image(y[1], n_fft, hop, r, frames=T + 1)
    strip = pg.spectrogram_strip_u8(y[1].copy(), n_fft, hop, img_mode='melif', mel_rows=M)
    assert strip.is_cuda and strip.is_contiguous() and tuple(strip.shape) == (2, M, T)
    _same_image(strip, want[:, :, 1:], before[:, :, 1:], 'spectrogram_strip_u8 melif')


def test_strip_dataset_from_waveforms():
    """DeviceStripDataset.from_waveforms(img_mode='melif'): strips of height mel_rows, batches equal to ops.real_batch_u8 on the
    materialised windows, bit for bit."""
    n_fft, M, hop = 64, 8, 16
    ys = [ref.signal(hop * 24, 2), ref.signal(hop * 9 + 5, 3)]
    kw = dict(img_mode='melif', mel_rows=M, sample_rate=22050, seed=1, mirror_augment=True, model_initial_depth=1)
    ds = pg.DeviceStripDataset.from_waveforms(ys, n_fft, hop, **kw)
    assert ds.shape == (4, 2, M, M) and ds.lengths == [24, 8]
    strips = [pg.spectrogram_strip_u8(y, n_fft, hop, img_mode='melif', mel_rows=M, sample_rate=22050) for y in ys]
    assert [tuple(s.shape) for s in strips] == [(2, M, 24), (2, M, 9)]
    r = ref.table(n_fft, M, 22050)
    want, before = ref.image(ys[1], n_fft, hop, r, frames=10)
    _same_image(strips[1], want[:, :, 1:], before[:, :, 1:], 'strip of the second waveform')
    twin = pg.DeviceStripDataset.from_waveforms(ys, n_fft, hop, **kw)       # the same stream: its crops are the first one's
    for n in (3, 4):
        idx, pos, flip = twin.draw_crops(n)
        stack = torch.stack([strips[m][:, :, u:u + M] for m, u in zip(idx.cpu().tolist(), pos.cpu().tolist())]).contiguous()
        want = pg.ops.real_batch_u8(stack, torch.arange(n, device='cuda'), flip, 0, ds.alpha, (0, 255), (-1, 1))
        got = ds.batch(n)
        assert tuple(got.shape) == (n, 2, M, M) and torch.equal(got, want)
    with pytest.raises(ValueError, match='waveform 1'):                     # 7 usable frames, a window needs mel_rows = 8 (not n_fft/2 = 32)
        pg.DeviceStripDataset.from_waveforms([ys[0], ref.signal(hop * 8 - 1, 4)], n_fft, hop, img_mode='melif', mel_rows=M)


@functools.lru_cache(maxsize=None)
def _generated(M, n_fft):
    """fp32 [2, 2, M, M] in (-1, 1): the 'melif' images of two test signals, as a generator trained on them would give."""
    hop = n_fft // 4
    r = ref.table(n_fft, M)
    u8 = np.stack([ref.image(ref.signal(hop * M + 7, 30 + b), n_fft, hop, r)[0] for b in range(2)])
    out = (u8.astype(np.float64) / 127.5 - 1).astype(np.float32)
    out.setflags(write=False)
    return out, hop


@pytest.mark.parametrize('M,n_fft', [(16, None), (32, 256)])
def test_savers_end_to_end(M, n_fft, tmp_path):
    from scipy.io import wavfile
    out, hop = _generated(M, 2 * M if n_fft is None else n_fft)
    r = ref.table(2 * M if n_fft is None else n_fft, M)
    kw = dict(resolution=2 * M, hop_length=hop, mode='melif', seed=11, n_fft=n_fft)
    host = pg.SoundSaver(str(tmp_path / 'host'), **kw)
    host(out.copy(), 7)
    dev = pg.DeviceSoundSaver(str(tmp_path / 'dev'), **kw)
    state = dev._rng.get_state()
    dev(torch.from_numpy(out.copy()).cuda(), 7)
    assert all(np.array_equal(a, b) for a, b in zip(state, dev._rng.get_state()))          # no random draws
    assert all(np.array_equal(a, b) for a, b in zip(state, host._rng.get_state()))
    names = sorted(os.listdir(str(tmp_path / 'dev')))
    assert names == sorted(os.listdir(str(tmp_path / 'host'))) == ['fakes_sound_000007_00.wav', 'fakes_sound_000007_01.wav']
    for i, name in enumerate(names):
        sr, wav = wavfile.read(os.path.join(str(tmp_path / 'dev'), name))
        sr_h, wav_h = wavfile.read(os.path.join(str(tmp_path / 'host'), name))
        want = ref.synthesise(out[i], hop, r)
        want = (want / np.abs(want).max()).repeat(2)
        print('melif %d^2 from %d bins, sample %d: host %.3e reference %.3e' % (M, r.bins, i, np.abs(wav - wav_h).max(), np.abs(wav - want).max()))
        assert sr == sr_h == 16000 and wav.dtype == np.float32 and wav.shape == wav_h.shape == want.shape
        assert np.abs(wav - wav_h).max() < 1e-5 and np.abs(wav - want).max() < 1e-5
    three = np.concatenate([out, out[:, :1]], axis=1)                      # further channels are ignored
    a = pg.DeviceSoundSaver(create_subdirs=False, **kw).to_waveforms(torch.from_numpy(out.copy()).cuda())
    b = pg.DeviceSoundSaver(create_subdirs=False, **kw).to_waveforms(three)
    assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (2, 2 * (M - 1) * hop) and torch.equal(a, b)


def test_launch_counts():
    """DeviceSoundSaver(mode='melif'): spectrum, pieces, overlap-add, normalise.  spectrogram_stack_u8: analysis and quantiser."""
    out, hop = _generated(16, 32)
    names = []

    def hook(fn, args, name):
        names.append(name)
        return fn(*args)
    x, y = torch.from_numpy(out.copy()).cuda(), _dev(_analysis_case(*ANALYSIS[3])[0])
    saver = pg.DeviceSoundSaver(create_subdirs=False, resolution=16, hop_length=hop, mode='melif')
    pg.mel_table(64, 8).on('cuda')                                          # (the table's upload is a copy, not a launch, and happens once)
    pg._lib.CALL_HOOK = hook
    try:
        saver.to_waveforms(x)
        pg.spectrogram_stack_u8(y, 64, 16, img_mode='melif', mel_rows=8)
    finally:
        pg._lib.CALL_HOOK = None
    assert names == ['pg_mel_spectrum_f64', 'pg_phase_pieces_f64', 'pg_overlap_add_f64', 'pg_wave_normalize_f32',
                     'pg_mel_analyse_f64', 'pg_phase_quantise_u8']


def test_argument_rejection():
    lib = pg._lib.load()
    E_ARG, E_UNSUP = -1, -3
    f64 = dict(dtype=torch.float64)
    t = pg.mel_table(32, 8)
    start, count, offset, weights, lower, frac = (a.data_ptr() for a in t.on('cuda'))
    y, lm, fr = torch.zeros(2, 120).cuda(), torch.zeros(2, 16, 16, **f64).cuda(), torch.zeros(2, 16, 16, **f64).cuda()
    img, spec = torch.zeros(2, 2, 16, 16).cuda(), torch.zeros(2, 16, 17, 2, **f64).cuda()
    Y, LM, FR, IM, S = [x.data_ptr() for x in (y, lm, fr, img, spec)]

    def analyse(y_=Y, ns=120, lm_=LM, fr_=FR, n_fft=32, hop=8, rows=8, frames=16, tab=(start, count, offset, weights)):
        return lib.pg_mel_analyse_f64(y_, ns, 2, lm_, fr_, n_fft, hop, rows, frames, tab[0], tab[1], tab[2], tab[3], None)

    def spectrum(i_=IM, s_=S, rows=8, H=16, W=16, tab=(lower, frac)):
        return lib.pg_mel_spectrum_f64(i_, s_, None, 2, rows, H, W, tab[0], tab[1], -1.0, 1.0, 0.0, -1.0, 127.5, 0.0, None)
    assert analyse() == 0 and spectrum() == 0                               # (the valid calls these are variations of)
    for n_fft in (4, 4096, 24):
        assert analyse(n_fft=n_fft, rows=2) == E_UNSUP and spectrum(H=n_fft // 2, rows=2) == E_UNSUP
    assert analyse(rows=1) == analyse(rows=17) == analyse(rows=0) == E_ARG
    assert spectrum(rows=1) == spectrum(rows=17) == E_ARG and spectrum(W=2048) == spectrum(W=12) == E_ARG
    assert analyse(ns=16, frames=1) == analyse(frames=17) == analyse(hop=0) == E_ARG
    assert analyse(y_=None) == analyse(lm_=None) == analyse(fr_=None) == spectrum(i_=None) == spectrum(s_=None) == E_ARG
    for k in range(4):
        assert analyse(tab=tuple(None if j == k else p for j, p in enumerate((start, count, offset, weights)))) == E_ARG
    assert spectrum(tab=(None, frac)) == spectrum(tab=(lower, None)) == E_ARG
    torch.cuda.synchronize()
    # the wrappers name the argument
    with pytest.raises(ValueError, match='table'):
        pg.mel_analyse(y, 64, 8, t)                                         # a table for another n_fft
    with pytest.raises(ValueError, match='table'):
        pg.mel_analyse(y, 32, 8, 'mel')
    with pytest.raises(ValueError, match='samples'):
        pg.mel_analyse(y[:, :16].contiguous(), 32, 8, t)
    with pytest.raises(ValueError, match='frames'):
        pg.mel_analyse(y, 32, 8, t, frames=17)
    with pytest.raises(ValueError, match='rows'):
        pg.mel_spectrum(img, t)                                             # 16 rows, the table has 8
    with pytest.raises(ValueError, match='images'):
        pg.mel_spectrum(torch.zeros(2, 2, 8, 16).cuda(), t)
    with pytest.raises(ValueError, match='images'):
        pg.mel_synthesise(torch.zeros(2, 1, 8, 8).cuda(), 8, t)
    with pytest.raises(ValueError, match='frames'):
        pg.spectrogram_stack_u8(y, 64, 16, img_mode='melif')                # 120 samples give 8 frames, the image needs 32
    with pytest.raises(ValueError):
        pg.DeviceSoundSaver(create_subdirs=False, mode='melif').to_waveforms(torch.zeros(1, 1, 16, 16).cuda())
    with pytest.raises(ValueError, match='padding'):                        # 15 frames every 8 samples: 120 samples, the padding is 128
        pg.DeviceSoundSaver(create_subdirs=False, mode='melif', n_fft=256, hop_length=8).to_waveforms(torch.zeros(1, 2, 16, 16).cuda())
