"""Griffin-Lim on the device (csrc/griffinlim.hip, ops.griffin_lim, sound.DeviceSoundSaver) against ``oracle/sound_steps.py`` in fp64 --
never against another kernel.  Inputs are seeded ``rand`` images in (-1, 1) and seeded ``randn`` starts.

The transform steps are held to 1e-9 x max|reference|, the bound tests/test_sound_steps.py uses between independent fp64 STFT
implementations; everything that has the same summands in the same order and no transform (overlap-add, normalisation, the 'abslog'
spectrum) is held bit-exact.  Every comparison prints its measured maximum before it asserts (docs/experiments_griffinlim.md)."""
import functools
import os

import numpy as np
import pytest
import torch

import pggan_amd as pg
from oracle import sound_steps as oss

pytestmark = pytest.mark.gpu

BOUND = 1e-9
# (H, hop, batch): the smallest shapes at which each piece can go wrong
CASES = [(4, 128, 1),       # n_fft 8 < hop: samples no frame covers are exactly 0
         (8, 3, 2),         # odd hop, many frames per sample
         (16, 8, 3),        # hop = n_fft/4, the exact-inverse regime
         (64, 128, 1),      # hop = n_fft: no overlap
         (128, 200, 2),     # hop neither a power of two nor a divisor
         (256, 128, 2),     # the sound configuration (n_fft 512: the largest size of the small-LDS instantiation)
         (1024, 128, 1)]    # n_fft 2048: the LDS and size limit, one round only
ITERATED = [c for c in CASES if c[0] != 1024]


class _Starts(object):
    """Stands in for the oracle's RNG: ``randn`` hands out the given start."""

    def __init__(self, x):
        self.x = x

    def randn(self, n):
        assert self.x.shape == (n,)
        return self.x.copy()


@functools.lru_cache(maxsize=None)
def _case(H, hop, batch):
    """Images, starts, the oracle's spectrum ([H + 1, W] per sample) and the oracle's pieces of the first round."""
    rs = np.random.RandomState(1000 * H + hop)
    img = (rs.rand(batch, H, H) * 2 - 1).astype(np.float32)
    nsamp = (H - 1) * hop
    x0 = rs.randn(batch, nsamp)
    mag = np.stack([oss.adjust_dynamic_range(np.vstack([im.astype(np.float64), np.zeros((1, H))]), (-1, 1), (0, 255)) for im in img])
    pieces = np.stack([_oracle_pieces(x0[b], mag[b], hop) for b in range(batch)])
    for a in (img, x0, mag, pieces):
        a.setflags(write=False)
    return img, x0, mag, pieces


def _oracle_pieces(x, mag, hop):
    """irfft(mag * exp(1j * angle(rfft(win * frame)))) * win * 2/3 per frame: the summands of oss.istft(mag * exp(1j angle(oss.stft(x))))."""
    n_fft = 2 * (mag.shape[0] - 1)
    S = oss.stft(x, n_fft, hop)
    assert S.shape == mag.shape
    full = mag * np.exp(1.0j * np.angle(S))
    win = oss.hann_periodic(n_fft) * (2.0 / 3.0)
    return np.stack([win * np.fft.irfft(full[:, t], n_fft) for t in range(full.shape[1])])


def _host_overlap_add(pieces, hop):
    frames, n_fft = pieces.shape
    y = np.zeros(n_fft + hop * (frames - 1))
    for t in range(frames):                                                # oss.istft's loop
        y[t * hop:t * hop + n_fft] += pieces[t]
    return y[n_fft // 2:-(n_fft // 2)]


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()                # (a writable copy: the shared references stay read-only)


def _spec_dev(mag):
    return _dev(mag.transpose(0, 2, 1))                                    # [n, W frames, H + 1 bins]


def _close(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print('%s: max|diff| %.3e, max|ref| %.3e, relative %.3e' % (what, err, scale, err / scale))
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err <= BOUND * scale, (what, err, scale)


@pytest.mark.parametrize('H,hop,batch', CASES)
def test_one_round_per_kernel(H, hop, batch):
    img, x0, mag, ref_pieces = _case(H, hop, batch)
    spec = _spec_dev(mag)
    pieces = pg.ops.gl_pieces(_dev(x0), spec, hop)
    assert tuple(pieces.shape) == (batch, H, 2 * H) and pieces.dtype == torch.float64
    _close(pieces, ref_pieces, 'pieces H=%d hop=%d' % (H, hop))
    # the overlap-add alone, fed the ORACLE's pieces: same summands, same order -> the same bits
    want = np.stack([_host_overlap_add(p, hop) for p in ref_pieces])
    got = pg.ops.overlap_add(_dev(ref_pieces), hop).cpu().numpy()
    assert got.shape == want.shape == x0.shape and np.array_equal(got, want)
    if hop > 2 * H:                                                        # samples between the frames
        assert (want == 0.0).sum() >= (hop - 2 * H) * (H - 1) and np.array_equal(got == 0.0, want == 0.0)
    # chained: one round of the oracle
    ref = np.stack([oss.griffin_lim(mag[b], hop, 1, _Starts(x0[b])) for b in range(batch)])
    _close(pg.ops.overlap_add(pieces, hop), ref, 'one round H=%d hop=%d' % (H, hop))
    _close(pg.ops.griffin_lim(_dev(img), _dev(x0), hop, 1), ref, 'griffin_lim(1) H=%d hop=%d' % (H, hop))


def test_zero_frames_take_phase_zero():
    """S == 0 -> phase factor (1, 0), np.angle(0) = 0.  The start is 0.0 over its first 3 n_fft samples, so the frames that lie wholly
    inside (the reflection at the front mirrors zeros onto zeros) transform to exactly 0."""
    H, hop, batch = 16, 8, 3
    img, x0, mag, _ = _case(H, hop, batch)
    n_fft = 2 * H
    x = x0.copy()
    x[:, :3 * n_fft] = 0.0
    zero_frames = [t for t in range(H) if t * hop + n_fft // 2 <= 3 * n_fft]              # frame t covers samples [t hop - N/2, t hop + N/2)
    assert len(zero_frames) == 11 and x.shape[1] - 3 * n_fft > n_fft // 2                 # the tail's reflection stays inside the non-zero part
    ref = np.stack([_oracle_pieces(x[b], mag[b], hop) for b in range(batch)])
    win = oss.hann_periodic(n_fft) * (2.0 / 3.0)
    for b in range(batch):
        for t in zero_frames:                                                              # ... the oracle's pieces there are irfft(mag * 1)
            assert np.array_equal(ref[b, t], win * np.fft.irfft(mag[b][:, t].astype(np.complex128), n_fft))
    got = pg.ops.gl_pieces(_dev(x), _spec_dev(mag), hop).cpu().numpy()
    _close(got[:, zero_frames], ref[:, zero_frames], 'pieces of all-zero frames')
    _close(got, ref, 'pieces next to all-zero frames')


@pytest.mark.parametrize('H,hop,batch,rounds', [c + (8,) for c in ITERATED] + [(128, 128, 2, 100)])
def test_whole_iteration(H, hop, batch, rounds):
    if (H, hop, batch) in CASES:
        img, x0, mag, _ = _case(H, hop, batch)
    else:
        rs = np.random.RandomState(H + hop + rounds)
        img, x0 = (rs.rand(batch, H, H) * 2 - 1).astype(np.float32), rs.randn(batch, (H - 1) * hop)
        mag = np.stack([oss.adjust_dynamic_range(np.vstack([im.astype(np.float64), np.zeros((1, H))]), (-1, 1), (0, 255)) for im in img])
    start = _dev(x0)
    got = pg.ops.griffin_lim(_dev(img), start, hop, rounds)
    ref = np.stack([oss.griffin_lim(mag[b], hop, rounds, _Starts(x0[b])) for b in range(batch)])
    assert got.dtype == torch.float64 and np.array_equal(start.cpu().numpy(), x0)          # the start is left unchanged
    _close(got, ref, 'griffin_lim(%d) H=%d hop=%d' % (rounds, H, hop))


@pytest.mark.parametrize('repeat', [1, 2, 4])
def test_wave_normalize_is_bit_exact(repeat):
    rs = np.random.RandomState(40 + repeat)
    x = rs.randn(3, 1531)
    x[1, 700] = -7.25                                                      # this sample's peak is negative
    x[2] *= 1e-3
    got = pg.ops.wave_normalize(_dev(x), repeat).cpu().numpy()
    want = np.stack([(s / np.abs(s).max()).repeat(repeat).astype(np.float32) for s in x])
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert got[1, 700 * repeat] == -1.0 and np.abs(got).max(axis=1).tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize('H,batch', [(4, 1), (16, 3), (128, 2)])
def test_spectrum(H, batch):
    rs = np.random.RandomState(H)
    img = (rs.rand(batch, H, H) * 2 - 1).astype(np.float32)
    pad = np.concatenate([img.astype(np.float64), np.zeros((batch, 1, H))], axis=1)
    for drange in ((-1, 1), (-1.5, 2.25)):
        got = pg.ops.gl_spectrum(_dev(img), 'abslog', drange).cpu().numpy()
        want = oss.adjust_dynamic_range(pad, drange, (0, 255)).transpose(0, 2, 1)
        assert got.shape == (batch, H, H + 1) and np.array_equal(got, want)       # padded row and transposed layout included
        assert np.all(got[:, :, H] == oss.adjust_dynamic_range(0.0, drange, (0, 255)))
        signed = oss.adjust_dynamic_range(pad, drange, (-1, 1))
        want = ((np.exp(np.abs(signed)) - 1) * np.sign(signed)).transpose(0, 2, 1)
        got = pg.ops.gl_spectrum(_dev(img[:, None]), 'reallog', drange).cpu().numpy()
        # exp comes from another math library: 4 ulp of exp(|v|), the value the two libraries differ in.  |v| <= 1, so exp(|v|) - 1 is
        # exact below 2 (Sterbenz) and rounds by at most half an ulp of a number that is smaller than exp(|v|) above it.
        ulps = np.abs(got - want) / np.spacing(np.exp(np.abs(signed))).transpose(0, 2, 1)
        print('reallog spectrum H=%d drange=%s: %.2f ulp of exp(|v|)' % (H, drange, ulps.max()))
        assert ulps.max() <= 4.0 and np.array_equal(np.sign(got), np.sign(want))
    assert np.all(pg.ops.gl_spectrum(_dev(img), 'abslog').cpu().numpy()[:, :, H] == 127.5)
    assert np.all(pg.ops.gl_spectrum(_dev(img), 'reallog').cpu().numpy()[:, :, H] == 0.0)


def _chirp(n, seed=0):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return (0.6 * np.sin(2 * np.pi * (200 + 900 * t) * t) + 0.05 * rs.randn(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _samples():
    """The [2,1,128,128] input of test_sound_saver_matches_oracle as float32."""
    img = oss.spectrogram_image(_chirp(128 * 140, 1), 256, 128)[0].astype(np.float64) / 127.5 - 1
    return np.stack([img, img[::-1].copy()])[:, None].astype(np.float32)


@pytest.mark.parametrize('mode', ['abslog', 'reallog', 'raw'])
def test_device_saver_end_to_end(mode, tmp_path):
    from scipy.io import wavfile
    out = _samples()
    kw = dict(resolution=256, hop_length=128, griffin_lim_iter=8, seed=11, mode=mode)
    pg.SoundSaver(str(tmp_path / 'host'), **kw)(out.copy(), 7)
    dev = pg.DeviceSoundSaver(str(tmp_path / 'dev'), **kw)
    dev(torch.from_numpy(out.copy()).cuda(), 7)
    names = sorted(os.listdir(str(tmp_path / 'dev')))
    assert names == sorted(os.listdir(str(tmp_path / 'host'))) == ['fakes_sound_000007_00.wav', 'fakes_sound_000007_01.wav']
    rng = np.random.RandomState(11)
    for i, name in enumerate(names):
        sr, wav = wavfile.read(os.path.join(str(tmp_path / 'dev'), name))
        sr_h, wav_h = wavfile.read(os.path.join(str(tmp_path / 'host'), name))
        ref = oss.image_to_sound(out[i, 0].astype(np.float64), mode, (-1, 1), 128, 8, rng).repeat(4 if mode == 'raw' else 2)
        print('%s sample %d: host %.3e oracle %.3e' % (mode, i, np.abs(wav - wav_h).max(), np.abs(wav - ref).max()))
        assert sr == sr_h == 16000 and wav.dtype == np.float32 and wav.shape == wav_h.shape == ref.shape
        assert np.abs(wav - wav_h).max() < 1e-5 and np.abs(wav - ref).max() < 1e-5
    # run to run: the same bits (no atomics, fixed summation order)
    a = pg.DeviceSoundSaver(create_subdirs=False, **kw).to_waveforms(torch.from_numpy(out.copy()).cuda())
    b = pg.DeviceSoundSaver(create_subdirs=False, **kw).to_waveforms(out)
    assert a.is_cuda and a.dtype == torch.float32 and torch.equal(a, b)


def test_stream_order():
    """to_waveforms on a side stream straight behind the generator pass that produces its input, without a synchronisation in between,
    gives what it gives after a full synchronise."""
    torch.manual_seed(3)
    G = pg.Generator((1, 1, 16, 16), latent_size=32, fmap_base=128, fmap_max=32).cuda()
    G.depth = 2
    z = torch.randn(3, 32).cuda()
    kw = dict(create_subdirs=False, resolution=32, hop_length=8, griffin_lim_iter=8, seed=4)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = G.forward(z)
        wav = pg.DeviceSoundSaver(**kw).to_waveforms(out)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 1, 16, 16) and tuple(wav.shape) == (3, 2 * 15 * 8)
    again = pg.DeviceSoundSaver(**kw).to_waveforms(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(wav, again) and float(wav.abs().max()) == 1.0


def test_argument_rejection():
    lib = pg._lib.load()
    E_ARG, E_UNSUP = -1, -3
    x, spec = torch.zeros(2, 120, dtype=torch.float64).cuda(), torch.zeros(2, 16, 17, dtype=torch.float64).cuda()
    pieces, img = torch.zeros(2, 16, 32, dtype=torch.float64).cuda(), torch.zeros(2, 16, 16).cuda()
    out, peak = torch.zeros(2, 120).cuda(), torch.zeros(2, dtype=torch.float64).cuda()
    X, S, P, I, O, K = [t.data_ptr() for t in (x, spec, pieces, img, out, peak)]
    assert lib.pg_gl_pieces_f64(X, 120, S, P, 32, 8, 16, 2, None) == 0                     # (the valid call these are variations of)
    for n_fft in (4096, 24, 4):
        assert lib.pg_gl_pieces_f64(X, 120, S, P, n_fft, 8, 16, 2, None) == E_UNSUP
        assert lib.pg_overlap_add_f64(P, X, 120, n_fft, 8, 16, 2, None) == E_UNSUP
    assert lib.pg_gl_spectrum_f64(I, S, 2, 2048, 16, -1.0, 127.5, 0.0, 0, None) == E_UNSUP
    assert lib.pg_gl_spectrum_f64(I, S, 2, 12, 16, -1.0, 127.5, 0.0, 0, None) == E_UNSUP
    assert lib.pg_gl_spectrum_f64(I, S, 2, 16, 16, -1.0, 127.5, 0.0, 2, None) == E_ARG     # no such mode
    assert lib.pg_gl_pieces_f64(X, 119, S, P, 32, 8, 16, 2, None) == E_ARG                 # nsamp != hop (frames - 1)
    assert lib.pg_gl_pieces_f64(X, 15, S, P, 32, 1, 16, 2, None) == E_ARG                  # nsamp <= n_fft/2
    assert lib.pg_overlap_add_f64(P, X, 121, 32, 8, 16, 2, None) == E_ARG
    assert lib.pg_gl_pieces_f64(X, 120, None, P, 32, 8, 16, 2, None) == E_ARG
    assert lib.pg_gl_pieces_f64(X, 120, S, None, 32, 8, 16, 2, None) == E_ARG
    assert lib.pg_overlap_add_f64(None, X, 120, 32, 8, 16, 2, None) == E_ARG and lib.pg_overlap_add_f64(P, None, 120, 32, 8, 16, 2, None) == E_ARG
    assert lib.pg_gl_spectrum_f64(None, S, 2, 16, 16, -1.0, 127.5, 0.0, 0, None) == E_ARG
    assert lib.pg_gl_spectrum_f64(I, None, 2, 16, 16, -1.0, 127.5, 0.0, 0, None) == E_ARG
    for args in ((None, O, 120, 1, 2, K), (X, None, 120, 1, 2, K), (X, O, 120, 1, 2, None), (X, O, 120, 0, 2, K), (X, O, 0, 1, 2, K)):
        assert lib.pg_wave_normalize_f32(*(args + (None,))) == E_ARG
    torch.cuda.synchronize()
    # the wrappers: host tensors, wrong dtypes and shapes are ValueErrors that name the argument
    with pytest.raises(ValueError, match='images'):
        pg.ops.griffin_lim(torch.zeros(2, 16, 16), x, 8, 1)
    with pytest.raises(ValueError, match='gl_pieces x'):
        pg.ops.gl_pieces(x.cpu(), spec, 8)
    with pytest.raises(ValueError, match='gl_pieces x'):
        pg.ops.gl_pieces(x[:, :119].contiguous(), spec, 8)
    with pytest.raises(ValueError, match='spec'):
        pg.ops.gl_pieces(x, spec.float(), 8)
    with pytest.raises(ValueError, match='n_fft'):
        pg.ops.gl_pieces(x, torch.zeros(2, 16, 13, dtype=torch.float64).cuda(), 8)
    with pytest.raises(ValueError, match='overlap_add out'):
        pg.ops.overlap_add(pieces, 8, out=x[:, :119].contiguous())
    with pytest.raises(ValueError, match='wave_normalize x'):
        pg.ops.wave_normalize(x.float())
    with pytest.raises(ValueError, match='gl_spectrum'):
        pg.ops.gl_spectrum(torch.zeros(2, 12, 12).cuda())
    with pytest.raises(ValueError):
        pg.DeviceSoundSaver(create_subdirs=False).to_waveforms(torch.zeros(1, 1, 64, 128).cuda())
