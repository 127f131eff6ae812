"""Magnitude + instantaneous frequency on the device (csrc/phase.hip, phase.py, sound.py's 'magif' modes) and the first two-channel
runs of the dataset and the training kernels, on the MI355X -- against tests/magif_ref.py (numpy fp64 on oracle/sound_steps.py),
host mode and the CPU oracle, never against another kernel.  "The test signal" is ``magif_ref.signal`` (tests/test_magif_host.py).

Bounds: 1e-9 x max|reference| between independent fp64 transforms (tests/test_griffinlim_gpu.py); a phase is weighed with its bin's
magnitude -- it is only as well defined as the bin is loud, and the DC and Nyquist rows sit exactly on +-pi where the sign of a zero
decides between -1 and +1 -- and no pixel is excluded.  Every comparison prints its measured maximum before it asserts
(docs/experiments_magif.md)."""
import functools
import os

import numpy as np
import pytest
import torch

import magif_ref as ref
import pggan_amd as pg
from conftest import rel_err
from helpers import reference_grads
from oracle import sound_steps as oss

pytestmark = pytest.mark.gpu

BOUND = 1e-9
# (n_fft, hop, batch)
ANALYSIS = [(8, 2, 1),
            (8, 128, 2),        # hop > n_fft
            (16, 3, 2),         # odd hop
            (64, 16, 3),
            (512, 128, 2),      # the sound configuration (the largest size of the small-LDS instantiation)
            (2048, 128, 1)]     # 1024 frames, the LDS limit
# (H, hop, batch, scale): as tests/test_griffinlim_gpu.py, plus one image scaled by 1.5 that reaches the clamp and |IF| > 1
SYNTHESIS = [(4, 128, 1, 1.0), (8, 3, 2, 1.0), (16, 8, 3, 1.0), (64, 128, 1, 1.0), (128, 200, 2, 1.0), (256, 128, 2, 1.0),
             (1024, 128, 1, 1.0), (16, 8, 2, 1.5)]


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()                # (a writable copy: the shared references stay read-only)


@functools.lru_cache(maxsize=None)
def _analysis_case(n_fft, hop, batch):
    """Signals with enough samples for n_fft/2 frames and a ragged rest, and the reference's S, logmag, ifreq per sample."""
    ns = hop * (n_fft // 2 - 1) + 5
    y = np.stack([ref.signal(ns, 100 * n_fft + hop + b) for b in range(batch)])
    S, logmag, ifreq = (np.stack(a) for a in zip(*[ref.analyse(y[b], n_fft, hop) for b in range(batch)]))
    for a in (y, S, logmag, ifreq):
        a.setflags(write=False)
    return y, S, logmag, ifreq


@functools.lru_cache(maxsize=None)
def _synthesis_case(H, hop, batch, scale):
    rs = np.random.RandomState(1000 * H + hop)
    img = ((rs.rand(batch, 2, H, H) * 2 - 1) * scale).astype(np.float32)
    spec = np.stack([ref.spectrum(im) for im in img])                      # [batch, H + 1, W]
    img.setflags(write=False)
    spec.setflags(write=False)
    return img, spec


def _close(got, want, what, scale=None):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max()) if scale is None else scale
    print('%s: max|diff| %.3e, max|ref| %.3e, relative %.3e' % (what, err, scale, err / scale))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= BOUND * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------------------ analysis
@pytest.mark.parametrize('crop', [False, True])
@pytest.mark.parametrize('n_fft,hop,batch', ANALYSIS)
def test_analysis(n_fft, hop, batch, crop):
    y, S, logmag, ifreq = _analysis_case(n_fft, hop, batch)
    bins, frames = (n_fft // 2, n_fft // 2) if crop else (n_fft // 2 + 1, S.shape[2])
    assert frames == (n_fft // 2 if crop else 1 + y.shape[1] // hop)
    lm, fr = pg.phase.analyse(_dev(y), n_fft, hop, bins if crop else None, frames if crop else None)
    assert lm.dtype == fr.dtype == torch.float64 and tuple(lm.shape) == tuple(fr.shape) == (batch, bins, frames)
    lm, fr = lm.cpu().numpy(), fr.cpu().numpy()
    S, logmag, ifreq = S[:, :bins, :frames], logmag[:, :bins, :frames], ifreq[:, :bins, :frames]
    M = float(np.abs(S).max())
    d = np.abs(fr - ifreq)
    dist = np.minimum(d, 2 - d) * np.abs(S)
    print('analysis n_fft=%d hop=%d bins=%d: |dlogmag| %.3e, IF circular distance x |S| %.3e, max|S| %.3e'
          % (n_fft, hop, bins, np.abs(lm - logmag).max(), dist.max(), M))
    assert np.isfinite(lm).all() and fr.min() >= -1.0 and fr.max() < 1.0
    assert np.abs(lm - logmag).max() <= BOUND * M and dist.max() <= BOUND * M


def test_analysis_of_silence_is_exactly_zero():
    lm, fr = pg.phase.analyse(torch.zeros(2, 300).cuda(), 64, 16)
    assert tuple(lm.shape) == (2, 33, 19) and not lm.any() and not fr.any()


@pytest.mark.parametrize('n_fft,hop,batch', ANALYSIS)
def test_uint8_image(n_fft, hop, batch):
    y, _, _, _ = _analysis_case(n_fft, hop, batch)
    h = n_fft // 2
    want = np.stack([ref.image(y[b], n_fft, hop) for b in range(batch)])
    got = pg.spectrogram_stack_u8(np.array(y), n_fft, hop)                 # (a writable copy: the shared references stay read-only)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (batch, 2, h, h)
    got = got.cpu().numpy()
    d0 = np.abs(got[:, 0].astype(int) - want[:, 0].astype(int))
    d1 = np.abs(got[:, 1].astype(int) - want[:, 1].astype(int))
    d1 = np.minimum(d1, 256 - d1)                                          # the 256-circle
    share = float((got != want).mean())
    print('uint8 image n_fft=%d hop=%d: channel 0 off by <= %d, channel 1 off by <= %d levels, %.3e of the pixels differ'
          % (n_fft, hop, d0.max(), d1.max(), share))
    assert d0.max() <= 1 and d1.max() <= 1 and share <= 1e-3
    # one waveform through the public single-image call; a two-column signal is mixed down first (sum / 2 in float32)
    one = pg.spectrogram_u8(np.array(y[0]), n_fft, hop, img_mode='magif')
    assert tuple(one.shape) == (2, h, h) and np.array_equal(one.cpu().numpy(), got[0])
    stereo = np.stack([y[0], y[-1]], axis=1)
    mono = (stereo.sum(axis=1) / 2).astype(np.float32)
    two = pg.spectrogram_u8(stereo, n_fft, hop, img_mode='magif', mag_range=(0.0, 3.0)).cpu().numpy()
    want2 = ref.image(mono, n_fft, hop, (0.0, 3.0))
    assert two.shape == want2.shape and float((two != want2).mean()) <= 1e-3


# ----------------------------------------------------------------------------------------------------------------- synthesis
@pytest.mark.parametrize('H,hop,batch,scale', SYNTHESIS)
def test_synthesis(H, hop, batch, scale):
    img, spec_ref = _synthesis_case(H, hop, batch, scale)
    W = H
    spec, c = pg.phase.spectrum(_dev(img), return_phase=True)
    assert spec.dtype == torch.complex128 and tuple(spec.shape) == (batch, W, H + 1) and tuple(c.shape) == (batch, H, W)
    # the running sum: (W - 1) 2^-53 sum|ifreq| per row bounds the error of ANY summation order
    worst = 0.0
    for b in range(batch):
        ifreq, c_ref = ref.running_sum(img[b], (-1, 1))
        bound = (W - 1) * 2.0 ** -53 * np.abs(ifreq).sum(axis=1, keepdims=True)
        err = np.abs(c[b].cpu().numpy() - c_ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (b, float((err / bound).max()))
    print('running sum H=%d: largest error %.3f of the bound' % (H, worst))
    if scale > 1.0:
        ifreq, _ = ref.running_sum(img[0], (-1, 1))
        assert np.abs(ifreq).max() > 1.0 and (spec_ref[0] == 0).sum() > H   # |IF| > 1 is a phase step like any other; clamped magnitudes
    _close(spec.cpu().numpy(), spec_ref.transpose(0, 2, 1), 'spec H=%d hop=%d' % (H, hop))
    assert not spec[:, :, H].cpu().numpy().any()                           # the Nyquist bin
    # pieces, fed the REFERENCE's spectrum
    pieces_ref = np.stack([ref.pieces(s) for s in spec_ref])
    got = pg.phase.pieces(_dev(np.ascontiguousarray(spec_ref.transpose(0, 2, 1))))
    assert tuple(got.shape) == (batch, W, 2 * H) and got.dtype == torch.float64
    _close(got, pieces_ref, 'pieces H=%d hop=%d' % (H, hop))
    # chained, after the (bit-exact, existing) overlap-add
    wave_ref = np.stack([oss.istft(s, hop) for s in spec_ref])
    wave = pg.phase.synthesise(_dev(img), hop)
    assert tuple(wave.shape) == (batch, hop * (W - 1))
    _close(wave, wave_ref, 'waveform H=%d hop=%d' % (H, hop))


def test_pieces_ignore_the_imaginary_parts_of_dc_and_nyquist():
    _, spec_ref = _synthesis_case(16, 8, 3, 1.0)
    s = np.ascontiguousarray(spec_ref.transpose(0, 2, 1))
    t = s.copy()
    t[:, :, 0] += 3.0j
    t[:, :, 16] = 0.25 - 2.0j
    s[:, :, 16] = 0.25
    assert torch.equal(pg.phase.pieces(_dev(s)), pg.phase.pieces(_dev(t)))
    _close(pg.phase.pieces(_dev(s)), np.stack([ref.pieces(x.T) for x in s]), 'pieces with a Nyquist bin')


def test_constant_phase_gives_an_exactly_real_spectrum():
    """IF = 0 (level 128) everywhere: c = 0, sinpi(0) = 0.  IF = -1 (level 0, e.g. an image of zeros under drange (0, 255)): c is a
    negative integer, sinpi of it is a zero, cospi alternates.  Both exactly."""
    rs = np.random.RandomState(8)
    img = rs.rand(2, 2, 16, 16).astype(np.float32) * 255
    for level, sign in ((128.0, lambda t: 1.0), (0.0, lambda t: -1.0 if t % 2 == 0 else 1.0)):
        img[:, 1] = level
        spec = pg.phase.spectrum(_dev(img), drange=(0, 255)).cpu().numpy()
        mag = np.expm1(oss.adjust_dynamic_range(img[:, 0].astype(np.float64), (0, 255), ref.default_mag_range(32)))
        assert not spec.imag.any()
        want = np.stack([mag[:, :, t] * sign(t) for t in range(16)], axis=1)           # [n, W, H]
        _close(spec.real[:, :, :16], want, 'real spectrum at level %d' % level)


# ---------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _generated(side):
    """fp32 [2, 2, side, side] in (-1, 1): the 'magif' images of two test signals, as a generator trained on them would give."""
    n_fft, hop = 2 * side, side // 2
    u8 = np.stack([ref.image(ref.signal(hop * side + 7, 30 + b), n_fft, hop) for b in range(2)])
    out = (u8.astype(np.float64) / 127.5 - 1).astype(np.float32)
    out.setflags(write=False)
    return out, hop


@pytest.mark.parametrize('side', [16, 128])
def test_savers_end_to_end(side, tmp_path):
    from scipy.io import wavfile
    out, hop = _generated(side)
    kw = dict(resolution=2 * side, hop_length=hop, mode='magif', seed=11)
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
        want = ref.synthesise(out[i], hop)
        want = (want / np.abs(want).max()).repeat(2)
        print('magif %d^2 sample %d: host %.3e reference %.3e' % (side, i, np.abs(wav - wav_h).max(), np.abs(wav - want).max()))
        assert sr == sr_h == 16000 and wav.dtype == np.float32 and wav.shape == wav_h.shape == want.shape
        assert np.abs(wav - wav_h).max() < 1e-5 and np.abs(wav - want).max() < 1e-5
    # the image really carries the signal: what comes back is the waveform the image was made from, to the quantiser's accuracy
    y = ref.signal(hop * side + 7, 30)[:hop * (side - 1)].astype(np.float64)
    x = ref.synthesise(out[0], hop)
    lo, hi = 2 * side, hop * (side - 1) - 2 * side
    corr = float(np.dot(x[lo:hi], y[lo:hi]) / np.sqrt(np.dot(x[lo:hi], x[lo:hi]) * np.dot(y[lo:hi], y[lo:hi])))
    print('magif %d^2: correlation of the resynthesised interior with the analysed waveform %.4f' % (side, corr))


def test_to_waveforms_takes_the_first_two_channels_and_is_deterministic():
    out, hop = _generated(16)
    kw = dict(create_subdirs=False, resolution=32, hop_length=hop, mode='magif')
    three = np.concatenate([out, out[:, :1]], axis=1)
    a = pg.DeviceSoundSaver(**kw).to_waveforms(torch.from_numpy(out.copy()).cuda())
    b = pg.DeviceSoundSaver(**kw).to_waveforms(three)
    assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (2, 2 * 15 * hop) and torch.equal(a, b)
    y = _dev(_analysis_case(64, 16, 3)[0])
    first, second = pg.phase.analyse(y, 64, 16), pg.phase.analyse(y, 64, 16)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert torch.equal(pg.phase.magif_u8(first[0], first[1], (0.0, 3.5)), pg.phase.magif_u8(second[0], second[1], (0.0, 3.5)))
    img = _dev(_synthesis_case(16, 8, 3, 1.0)[0])
    assert torch.equal(torch.view_as_real(pg.phase.spectrum(img)), torch.view_as_real(pg.phase.spectrum(img)))
    assert torch.equal(pg.phase.synthesise(img, 8), pg.phase.synthesise(img, 8))


def test_launch_counts():
    """DeviceSoundSaver(mode='magif'): spectrum, pieces, overlap-add, normalise.  spectrogram_stack_u8: analysis and quantiser."""
    out, hop = _generated(16)
    names = []

    def hook(fn, args, name):
        names.append(name)
        return fn(*args)
    x, y = torch.from_numpy(out.copy()).cuda(), _dev(_analysis_case(64, 16, 3)[0])
    saver = pg.DeviceSoundSaver(create_subdirs=False, resolution=16, hop_length=hop, mode='magif')
    pg._lib.CALL_HOOK = hook
    try:
        saver.to_waveforms(x)
        pg.spectrogram_stack_u8(y, 64, 16)
    finally:
        pg._lib.CALL_HOOK = None
    assert names == ['pg_phase_spectrum_f64', 'pg_phase_pieces_f64', 'pg_overlap_add_f64', 'pg_wave_normalize_f32',
                     'pg_phase_analyse_f64', 'pg_phase_quantise_u8']


def test_stream_order():
    """to_waveforms on a side stream straight behind the two-channel generator pass that produces its input, and the analysis behind the
    copy that produces its input, without a synchronisation in between, give what they give after a full synchronise."""
    torch.manual_seed(3)
    G = pg.Generator((1, 2, 16, 16), latent_size=32, fmap_base=128, fmap_max=32).cuda()
    G.depth = 2
    z = torch.randn(3, 32).cuda()
    y = _dev(_analysis_case(64, 16, 3)[0])
    kw = dict(create_subdirs=False, resolution=32, hop_length=8, mode='magif')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = G.forward(z)
        wav = pg.DeviceSoundSaver(**kw).to_waveforms(out)
        y2 = y * 0.5
        img = pg.spectrogram_stack_u8(y2, 64, 16)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 2, 16, 16) and tuple(wav.shape) == (3, 2 * 15 * 8)
    again = pg.DeviceSoundSaver(**kw).to_waveforms(out.clone())
    img_again = pg.spectrogram_stack_u8(y2.clone(), 64, 16)
    torch.cuda.synchronize()
    assert torch.equal(wav, again) and float(wav.abs().max()) == 1.0 and torch.equal(img, img_again)


def test_argument_rejection():
    lib = pg._lib.load()
    E_ARG, E_UNSUP = -1, -3
    f64 = dict(dtype=torch.float64)
    y, lm, fr = torch.zeros(2, 120).cuda(), torch.zeros(2, 17, 16, **f64).cuda(), torch.zeros(2, 17, 16, **f64).cuda()
    u8, img = torch.zeros(2, 2, 17, 16, dtype=torch.uint8).cuda(), torch.zeros(2, 2, 16, 16).cuda()
    spec, pieces = torch.zeros(2, 16, 17, 2, **f64).cuda(), torch.zeros(2, 16, 32, **f64).cuda()
    Y, LM, FR, U, IM, S, PC = [t.data_ptr() for t in (y, lm, fr, u8, img, spec, pieces)]
    analyse = lambda y_, ns, lm_, fr_, n_fft, hop=8, bins=17, frames=16: lib.pg_phase_analyse_f64(y_, ns, 2, lm_, fr_, n_fft, hop, bins, frames, None)
    spectrum = lambda i_, s_, H, W=16: lib.pg_phase_spectrum_f64(i_, s_, None, 2, H, W, -1.0, 1.0, 0.0, -1.0, 127.5, 0.0, None)
    assert analyse(Y, 120, LM, FR, 32) == 0 and spectrum(IM, S, 16) == 0                     # (the valid calls these are variations of)
    assert lib.pg_phase_pieces_f64(S, PC, 32, 16, 2, None) == 0
    assert lib.pg_phase_quantise_u8(LM, FR, U, 2, 17 * 16, 0.0, 3.0, None) == 0
    for n_fft in (4, 4096, 24):
        assert analyse(Y, 120, LM, FR, n_fft, bins=1) == E_UNSUP
        assert lib.pg_phase_pieces_f64(S, PC, n_fft, 16, 2, None) == E_UNSUP
        assert spectrum(IM, S, n_fft // 2) == E_UNSUP
    assert analyse(Y, 16, LM, FR, 32, frames=1) == E_ARG                                   # nsamp <= n_fft/2
    assert analyse(Y, 120, LM, FR, 32, bins=18) == E_ARG and analyse(Y, 120, LM, FR, 32, frames=17) == E_ARG
    assert analyse(Y, 120, LM, FR, 32, hop=0) == E_ARG
    assert analyse(None, 120, LM, FR, 32) == analyse(Y, 120, None, FR, 32) == analyse(Y, 120, LM, None, 32) == E_ARG
    assert spectrum(None, S, 16) == spectrum(IM, None, 16) == E_ARG and spectrum(IM, S, 16, W=12) == E_ARG
    assert spectrum(IM, S, 16, W=2048) == E_ARG
    assert lib.pg_phase_pieces_f64(None, PC, 32, 16, 2, None) == lib.pg_phase_pieces_f64(S, None, 32, 16, 2, None) == E_ARG
    assert lib.pg_phase_pieces_f64(S, PC, 32, 0, 2, None) == E_ARG
    for args in ((None, FR, U), (LM, None, U), (LM, FR, None)):
        assert lib.pg_phase_quantise_u8(*(args + (2, 17 * 16, 0.0, 3.0, None))) == E_ARG
    assert lib.pg_phase_quantise_u8(LM, FR, U, 2, 17 * 16, 1.0, 1.0, None) == E_ARG
    torch.cuda.synchronize()
    # the wrappers name the argument
    with pytest.raises(ValueError, match='n_fft'):
        pg.phase.analyse(y, 48, 8)
    with pytest.raises(ValueError, match='samples'):
        pg.phase.analyse(y[:, :16].contiguous(), 32, 8)
    with pytest.raises(ValueError, match='bins'):
        pg.phase.analyse(y, 32, 8, bins=18)
    with pytest.raises(ValueError, match='magif_u8'):
        pg.phase.magif_u8(lm, fr[:, :16].contiguous(), (0.0, 1.0))
    with pytest.raises(ValueError, match='mag_range'):
        pg.phase.magif_u8(lm, fr, (1.0, 0.0))
    with pytest.raises(ValueError, match='images'):
        pg.phase.spectrum(torch.zeros(2, 2, 16, 32).cuda())
    with pytest.raises(ValueError, match='images'):
        pg.phase.synthesise(torch.zeros(2, 1, 16, 16).cuda(), 8)
    with pytest.raises(ValueError, match='frames'):
        pg.spectrogram_stack_u8(y, 64, 16)                                                # 120 samples give 8 frames, the image needs 32
    with pytest.raises(ValueError):
        pg.DeviceSoundSaver(create_subdirs=False, mode='magif').to_waveforms(torch.zeros(1, 1, 16, 16).cuda())


# -------------------------------------------------------------------------------------------------------------- two channels
def test_two_channel_dataset_matches_host_mode():
    rs = np.random.RandomState(21)
    stack = rs.randint(0, 256, size=(5, 2, 16, 16)).astype(np.uint8)
    stack[4, 1] = 255
    for pyramid in ('chain', 'direct'):
        for depth in (2, 1, 0):                                            # depth differences 0, 1, 2 of 'direct'
            for alpha in (1.0, 0.5):
                kw = dict(model_initial_depth=depth, alpha=alpha, pyramid=pyramid, mirror_augment=True, seed=4, two_channel=True)
                dev, host = pg.DeviceImageDataset(stack, **kw), pg.DeviceImageDataset(stack, device='cpu', **kw)
                a, b = dev.batch(7), host.batch(7)
                assert a.is_cuda and tuple(a.shape) == tuple(b.shape) == (7, 2, 4 << depth, 4 << depth)
                assert np.array_equal(a.cpu().numpy(), b.numpy()), (pyramid, depth, alpha)
                assert np.array_equal(dev.level_stack().cpu().numpy(), host.level_stack().numpy())
    lib, out = pg._lib.load(), torch.empty(2 * 2 * 16 * 16, device='cuda')
    s, i = _dev(stack), torch.tensor([0, 4]).cuda()
    call = lambda src, M, S, dd, ix, n, o: lib.pg_real_batch_2ch_u8(src, M, S, dd, ix, None, n, o, 1.0, 0.0, 255.0, -1.0, 1.0, None)
    assert call(s.data_ptr(), 5, 16, 0, i.data_ptr(), 2, out.data_ptr()) == 0
    assert call(None, 5, 16, 0, i.data_ptr(), 2, out.data_ptr()) == call(s.data_ptr(), 5, 16, 0, None, 2, out.data_ptr()) == -1
    assert call(s.data_ptr(), 5, 16, 0, i.data_ptr(), 2, None) == call(s.data_ptr(), 0, 16, 0, i.data_ptr(), 2, out.data_ptr()) == -1
    assert call(s.data_ptr(), 5, 12, 0, i.data_ptr(), 2, out.data_ptr()) == call(s.data_ptr(), 5, 16, 4, i.data_ptr(), 2, out.data_ptr()) == -2
    torch.cuda.synchronize()


def test_two_channel_training_iteration(oracle):
    """One full iteration -- D step with the gradient penalty, Adam, G step, Adam -- of a two-channel 16^2 network with the narrow feature
    maps of the tiny fixtures, during a fade-in, against oracle.train_iteration.  Bounds: those of tests/test_e2e_gpu.py for its one-
    and three-channel networks (OUT_TOL for outputs and losses; per-tensor relative L2 1e-2 and max-norm 3e-2, global L2 4e-3 for the
    gradients against the oracle; 5e-3 relative max-norm per tensor for the weights after Adam steps)."""
    OUT_TOL, GRAD_L2_TOL, GRAD_MAX_TOL, GRAD_GLOBAL_L2_TOL, WEIGHT_TOL = 2e-4, 1e-2, 3e-2, 4e-3, 5e-3
    torch.manual_seed(5)
    shape, kw, depth, alpha, n, lr = (1, 2, 16, 16), dict(fmap_base=128, fmap_max=32), 2, 0.6, 4, 0.001
    G = pg.Generator(shape, latent_size=32, **kw)
    D = pg.Discriminator(shape, **kw)
    gp, dp = G.reference_state_dict(), D.reference_state_dict()
    G.cuda()
    D.cuda()
    cfg = oracle.NetCfg(16, 2, latent_size=32, **kw)
    G.depth = D.depth = depth
    G.alpha = D.alpha = alpha
    real, z_d, z_g, mix = oracle.synthetic_batch(9, n, 2, 16, 32)
    og, od = oracle.AdamState(), oracle.AdamState()
    d_ref, g_ref = oracle.train_iteration(gp, dp, cfg, og, od, real, z_d, z_g, mix, depth, alpha, lr, lr)

    def grads(mine, want, what):
        num = den = worst_l2 = worst_max = 0.0
        assert sorted(mine) == sorted(want)
        for k, r in want.items():
            a = mine[k].detach().cpu().reshape(r.shape).double()
            l2, mx = float((a - r.double()).norm() / (r.double().norm() + 1e-30)), rel_err(a, r)
            worst_l2, worst_max = max(worst_l2, l2), max(worst_max, mx)
            num, den = num + float((a - r.double()).pow(2).sum()), den + float(r.double().pow(2).sum())
        glob = (num / den) ** 0.5
        print('%s: worst per-tensor rel-L2 %.2e, worst rel-max %.2e, global rel-L2 %.2e' % (what, worst_l2, worst_max, glob))
        assert worst_l2 < GRAD_L2_TOL and worst_max < GRAD_MAX_TOL and glob < GRAD_GLOBAL_L2_TOL, what

    opt_g = pg.FusedAdam(G.parameters(), lr, betas=(0.0, 0.99))
    opt_d = pg.FusedAdam(D.parameters(), lr, betas=(0.0, 0.99))
    pg.wgan_gp_loss.set_mixing_factors(mix)
    d_cost, d_real_loss, d_fake_loss = pg.wgan_gp_D_loss(D, G, real.cuda(), z_d.cuda())
    d_cost.backward()
    errs = [rel_err(d_cost, d_ref['D_cost']), rel_err(d_real_loss, d_ref['D_real_loss']), rel_err(d_fake_loss, d_ref['D_fake_loss'])]
    print('two-channel D step: D_cost %.6f (oracle %.6f), relative errors of cost / real / fake %.2e %.2e %.2e'
          % (float(d_cost), float(d_ref['D_cost']), errs[0], errs[1], errs[2]))
    assert max(errs) < OUT_TOL
    grads(reference_grads(D), d_ref['grads'], 'two-channel D gradients')
    opt_d.step()
    g_cost = pg.wgan_gp_G_loss(G, D, z_g.cuda())
    g_cost.backward()
    e = rel_err(g_cost, g_ref['G_cost'])
    print('two-channel G step: G_cost %.6f (oracle %.6f), relative error %.2e' % (float(g_cost), float(g_ref['G_cost']), e))
    assert e < OUT_TOL and rel_err(G(z_g.cuda()).cpu(), g_ref['fake']) < OUT_TOL
    grads(reference_grads(G), g_ref['grads'], 'two-channel G gradients')
    opt_g.step()
    worst = 0.0
    for net, want in ((G, gp), (D, dp)):
        for k, v in net.reference_state_dict().items():
            if torch.is_tensor(v):
                worst = max(worst, rel_err(v.cpu(), want[k]))
                assert rel_err(v.cpu(), want[k]) < WEIGHT_TOL, k
    print('two-channel weights after the Adam steps: worst relative max-norm error %.2e' % worst)
