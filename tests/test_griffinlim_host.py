"""Host logic of ``sound.DeviceSoundSaver`` and ``ops.griffin_lim`` on CPU tensors: the four kernels of csrc/griffinlim.hip replaced by
tests/emu_sound.py's numpy statement of their contracts (include/pggan_hip.h).  Held against the host ``SoundSaver`` and against
``oracle/sound_steps.py``; the kernels themselves are checked on the device (tests/test_griffinlim_gpu.py)."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import emu_sound

import pggan_amd as pg
from oracle import sound_steps as oss

WAV_BOUND = 1e-5                       # test_sound_saver_matches_oracle's bound on float32 WAV data


def _chirp(n, seed=0):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return (0.6 * np.sin(2 * np.pi * (200 + 900 * t) * t) + 0.05 * rs.randn(n)).astype(np.float32)


@pytest.fixture(scope='module')
def samples():
    """The [2,1,128,128] input of test_sound_saver_matches_oracle, float32 as G delivers it."""
    img = oss.spectrogram_image(_chirp(128 * 140, 1), 256, 128)[0].astype(np.float64) / 127.5 - 1
    out = np.stack([img, img[::-1].copy()])[:, None].astype(np.float32)
    return out


@pytest.fixture()
def emu(monkeypatch):
    calls = []
    for name in ('gl_spectrum', 'gl_pieces', 'overlap_add', 'wave_normalize'):
        def logged(*a, _f=getattr(emu_sound, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(pg.ops, name, logged)
    monkeypatch.setattr(pg.sound, '_to_device', lambda t: t)
    yield calls


def _wavs(path):
    return {n: wavfile.read(os.path.join(str(path), n)) for n in sorted(os.listdir(str(path)))}


def test_device_saver_writes_what_the_host_saver_and_the_oracle_give(emu, samples, tmp_path):
    kw = dict(resolution=256, hop_length=128, griffin_lim_iter=8, seed=11)
    pg.SoundSaver(str(tmp_path / 'host'), **kw)(samples, 7)
    pg.DeviceSoundSaver(str(tmp_path / 'dev'), **kw)(torch.from_numpy(samples.copy()), 7)
    host, dev = _wavs(tmp_path / 'host'), _wavs(tmp_path / 'dev')
    assert list(dev) == list(host) == ['fakes_sound_000007_00.wav', 'fakes_sound_000007_01.wav']
    rng = np.random.RandomState(11)
    for i, name in enumerate(dev):
        (sr, wav), (sr_h, wav_h) = dev[name], host[name]
        ref = oss.image_to_sound(samples[i, 0], 'abslog', (-1, 1), 128, 8, rng).repeat(2)
        assert sr == sr_h == 16000 and wav.dtype == np.float32 and wav.shape == wav_h.shape == ref.shape == (2 * 127 * 128,)
        assert np.abs(wav - wav_h).max() < WAV_BOUND
        assert np.abs(wav - ref / np.abs(ref).max()).max() < WAV_BOUND
        assert np.abs(wav).max() == 1.0
    assert emu == ['gl_spectrum'] + ['gl_pieces', 'overlap_add'] * 8 + ['wave_normalize']       # 1 + 2 rounds launches, one batch


def test_padded_row_is_adjusted_like_the_rest(emu, samples):
    img = torch.from_numpy(samples.copy())
    spec = pg.ops.gl_spectrum(img, 'abslog', (-1, 1)).numpy()
    assert spec.shape == (2, 128, 129) and spec.dtype == np.float64
    assert np.all(spec[:, :, 128] == oss.adjust_dynamic_range(0.0, (-1, 1), (0, 255))) and spec[0, 0, 128] == 127.5
    want = oss.adjust_dynamic_range(samples[:, 0].astype(np.float64), (-1, 1), (0, 255))
    assert np.array_equal(spec[:, :, :128], want.transpose(0, 2, 1))
    assert np.all(pg.ops.gl_spectrum(img, 'abslog', (0, 255)).numpy()[:, :, 128] == 0.0)
    real = pg.ops.gl_spectrum(img, 'reallog', (-1, 1)).numpy()
    assert np.all(real[:, :, 128] == 0.0) and np.abs(real[:, :, :128]).max() > 0.5
    assert np.all(pg.ops.gl_spectrum(img, 'reallog', (0, 1)).numpy()[:, :, 128] == -(np.exp(1.0) - 1))   # 0 -> -1 under (0,1) -> (-1,1)


@pytest.mark.parametrize('mode,resolution,repeat', [('reallog', 128, 1), ('reallog', 256, 2), ('raw', 128, 1), ('raw', 256, 4)])
def test_reallog_and_raw_against_the_oracle(emu, samples, tmp_path, mode, resolution, repeat):
    saver = pg.DeviceSoundSaver(str(tmp_path), mode=mode, resolution=resolution, hop_length=128, seed=3)
    wav = saver.to_waveforms(samples)                                      # a numpy array is uploaded
    nsamp = 128 * 128 if mode == 'raw' else 127 * 128
    assert torch.is_tensor(wav) and wav.dtype == torch.float32 and tuple(wav.shape) == (2, nsamp * repeat)
    for i in range(2):
        ref = oss.image_to_sound(samples[i, 0].astype(np.float64), mode, (-1, 1), 128, 0, None).repeat(repeat)
        assert np.abs(wav[i].numpy() - ref).max() < WAV_BOUND
    assert emu == (['wave_normalize'] if mode == 'raw' else ['gl_spectrum', 'gl_pieces', 'overlap_add', 'wave_normalize'])
    saver(samples, 'x')
    assert sorted(os.listdir(str(tmp_path))) == ['fakes_sound_x_00.wav', 'fakes_sound_x_01.wav']
    sr, data = wavfile.read(os.path.join(str(tmp_path), 'fakes_sound_x_01.wav'))
    assert np.array_equal(data, wav[1].numpy())                            # output_wav's own normalisation is the identity


def test_abslog_repeat_and_seed(emu, samples):
    a = pg.DeviceSoundSaver(create_subdirs=False, resolution=256, griffin_lim_iter=2, seed=5).to_waveforms(samples).numpy()
    b = pg.DeviceSoundSaver(create_subdirs=False, resolution=128, griffin_lim_iter=2, seed=5).to_waveforms(samples).numpy()
    c = pg.DeviceSoundSaver(create_subdirs=False, resolution=128, griffin_lim_iter=2, seed=6).to_waveforms(samples).numpy()
    assert a.shape == (2, 2 * 127 * 128) and np.array_equal(a, b.repeat(2, axis=1)) and not np.array_equal(b, c)
    # the draws are the host saver's: one randn(nsamp) per sample in sample order
    saver = pg.DeviceSoundSaver(create_subdirs=False, resolution=128, griffin_lim_iter=0, seed=5)
    rs = np.random.RandomState(5)
    want = np.stack([rs.randn(127 * 128) for _ in range(2)])
    assert np.array_equal(saver.to_waveforms(samples).numpy(), (want / np.abs(want).max(axis=1, keepdims=True)).astype(np.float32))


def test_verbose_prints_the_host_savers_line(emu, samples, capsys):
    pg.DeviceSoundSaver(create_subdirs=False, griffin_lim_iter=2, seed=5, verbose=True).to_waveforms(samples[:1])
    dev = capsys.readouterr().out
    s = pg.SoundSaver(create_subdirs=False, griffin_lim_iter=2, seed=5, verbose=True)
    s.image_to_sound(samples[0, 0])
    host = capsys.readouterr().out
    prefix = 'Griffin-Lim: change of the signal in this round (L2) = '
    assert len(dev.splitlines()) == 2 and all(l.startswith(prefix) for l in dev.splitlines() + host.splitlines())
    value = lambda l: float(l[len(prefix):])                               # noqa: E731
    assert np.allclose([value(l) for l in dev.splitlines()], [value(l) for l in host.splitlines()], rtol=1e-5, atol=0)


def test_value_errors(emu, samples):
    mk = lambda **kw: pg.DeviceSoundSaver(create_subdirs=False, griffin_lim_iter=1, seed=1, **kw)      # noqa: E731
    z = lambda *shape: np.zeros(shape, np.float32)                                                      # noqa: E731
    for bad in (z(1, 1, 128, 64), z(1, 1, 64, 128),                        # not square
                z(1, 1, 48, 48), z(1, 1, 2, 2), z(1, 1, 2048, 2048),       # no power of two / outside 4 .. 1024
                z(1, 128, 128), z(0, 1, 128, 128)):
        with pytest.raises(ValueError):
            mk().to_waveforms(bad)
    with pytest.raises(ValueError):                                        # 15 * 1 = 15 samples <= n_fft/2 = 16
        mk(hop_length=1).to_waveforms(z(1, 1, 16, 16))
    with pytest.raises(ValueError):
        mk(mode='reallog', hop_length=1).to_waveforms(z(1, 1, 16, 16))
    with pytest.raises(ValueError):
        mk(mode='phase').to_waveforms(samples)
    assert emu == []                                                       # all refused before anything is launched
    with pytest.raises(ValueError):
        pg.ops.griffin_lim(torch.from_numpy(samples.copy()), None, 128, 1)        # 'abslog' without starts


def test_real_wrappers_refuse_host_tensors(samples):
    """No CPU path: without the emulation every wrapper names the host tensor it was given."""
    img, x = torch.from_numpy(samples.copy()), torch.zeros(2, 127 * 128, dtype=torch.float64)
    spec = torch.zeros(2, 128, 129, dtype=torch.float64)
    for call in (lambda: pg.ops.gl_spectrum(img), lambda: pg.ops.gl_pieces(x, spec, 128), lambda: pg.ops.wave_normalize(x),
                 lambda: pg.ops.overlap_add(torch.zeros(2, 128, 256, dtype=torch.float64), 128),
                 lambda: pg.ops.griffin_lim(img, x, 128, 1)):
        with pytest.raises(ValueError, match='device tensor'):
            call()


def test_names_and_signatures():
    assert pg.DeviceSoundSaver.accepts_device_tensors is True and issubclass(pg.DeviceSoundSaver, pg.SoundSaver)
    assert not getattr(pg.SoundSaver, 'accepts_device_tensors', False)                       # the host saver still gets host arrays
    assert 'DeviceSoundSaver' in pg.__all__ and pg.sound.DeviceSoundSaver is pg.DeviceSoundSaver
    P, I, L, D = pg._lib.P, pg._lib.I, pg._lib.L, pg._lib.D
    sig = pg._lib.SIGNATURES
    assert sig['pg_gl_spectrum_f64'] == [P, P, I, I, I, D, D, D, I, P]
    assert sig['pg_gl_pieces_f64'] == [P, L, P, P, I, I, I, I, P]
    assert sig['pg_overlap_add_f64'] == [P, P, L, I, I, I, I, P]
    assert sig['pg_wave_normalize_f32'] == [P, P, L, I, I, P, P]
    assert pg._lib.ABI_VERSION == 27                                                         # additive: the version stays


class _Z(object):
    def __init__(self, z):
        self.z = z

    def cuda(self):
        return self.z


class _G(object):
    def forward(self, z):
        return z


class _Trainer(object):
    parallel, g_ema, cur_nimg = None, None, 12000
    G = _G()


def test_output_generator_hands_the_device_tensor_through(emu, samples, tmp_path):
    """plugins.OutputGenerator needs no change: a post-processor with ``accepts_device_tensors`` gets G's tensor itself, the host
    ``SoundSaver`` beside it a numpy copy."""
    out = torch.from_numpy(samples.copy())
    seen = []

    class Spy(pg.DeviceSoundSaver):
        def to_waveforms(self, output):
            seen.append(output)
            return super(Spy, self).to_waveforms(output)

    class HostSpy(pg.SoundSaver):
        def __call__(self, output, description):
            seen.append(output)

    og = pg.OutputGenerator(lambda n: _Z(out), [Spy(str(tmp_path), hop_length=128, griffin_lim_iter=1, seed=2), HostSpy(str(tmp_path))],
                            samples_count=2)
    og.register(_Trainer())
    og.epoch(1)
    assert seen[0] is out and isinstance(seen[1], np.ndarray)
    assert sorted(os.listdir(str(tmp_path))) == ['fakes_sound_000012_00.wav', 'fakes_sound_000012_01.wav']
