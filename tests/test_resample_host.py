"""Rate conversion on the host (pggan-pytorch_amd/sound.py: ``resample_table``, ``resample(device='cpu')``, ``resampled_length``,
``load_wav``): the table and the numpy twin against the independent restatement of tests/resample_ref.py with ``==``, the quality of
the definition on sines, the WAV reader, every ValueError of the new arguments and the binding table of
include/pggan_hip_resample.h.  Host tests: no GPU, no shared library."""
import os
import re

import numpy as np
import pytest
from scipy.io import wavfile

import resample_ref as ref

import pggan_amd as pg

sound, _lib = pg.sound, pg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RATES = [(44100, 16000), (48000, 16000), (16000, 44100), (3, 2), (2, 3), (7, 5), (1, 3)]
LMT = {(44100, 16000): (160, 441, 374), (48000, 16000): (1, 3, 406), (16000, 44100): (441, 160, 136)}
# (rate_in, rate_out, nsamp) of the GPU tier's tiny shapes: signals shorter than the filter, L = 1 and M = 1
TINY = [(3, 2, 1), (3, 2, 5), (2, 3, 7), (5, 7, 33), (3, 1, 100), (1, 3, 50)]


@pytest.fixture(scope='module')
def tables():
    return {rates: ref.table(*rates) for rates in RATES}


@pytest.mark.parametrize('rates', RATES)
def test_table_is_the_formula(tables, rates):
    t = sound.resample_table(*rates)
    want = tables[rates]
    assert (t.L, t.M) == ref.ratio(*rates) and t.taps.shape == want.shape == (t.L, t.T) and t.taps.dtype == np.float64
    assert np.array_equal(t.taps, want)
    if rates in LMT:
        assert (t.L, t.M, t.T) == LMT[rates]
    assert t.T % 2 == 0 and t.taps.nbytes == 8 * t.L * t.T
    dev = np.abs(t.taps.sum(axis=1) - 1.0).max()
    print('%d -> %d: largest deviation of a phase row\'s sum from 1: %.3e' % (rates + (dev,)))
    assert dev <= 1e-6
    # The filter is even in tau = (r + L (half - 1 - j)) / L, and the integers make the mirror image exact.  -tau(r, j) is
    # tau(L - r, T - 1 - j) for 0 < r < L and tau(0, T - 2 - j) for r = 0, whose last tap sits at tau = -half, outside the window.
    # (The issue writes T - 2 - j for 0 < r < L as well; that is the index of r = 0, and one tap off for the others.)
    L, T = t.L, t.T
    for r in range(1, L):
        assert np.array_equal(t.taps[r], t.taps[L - r, ::-1]), r
    assert np.array_equal(t.taps[0, :T - 1], t.taps[0, T - 2::-1]) and t.taps[0, T - 1] == 0.0
    assert sound.resample_table(*rates) is t                                  # memoised
    assert not t.taps.flags.writeable


def test_table_parameters_and_custom_table():
    a = sound.resample_table(3, 2, zeros=8, rolloff=0.9, beta=6.0)
    assert np.array_equal(a.taps, ref.table(3, 2, 8, 0.9, 6.0)) and a.T == 2 * int(np.ceil(8 / (0.9 * 2 / 3)))
    assert a is not sound.resample_table(3, 2)
    t = sound.ResampleTable(3, 4, np.arange(12.0).reshape(3, 4))
    assert (t.L, t.M, t.T) == (3, 4, 4)
    for L, M, taps in [(3, 4, np.zeros((3, 5))), (3, 4, np.zeros((2, 4))), (3, 4, np.zeros(12)), (3, 4, np.full((3, 4), np.nan)),
                       (3, 4, np.full((3, 4), np.inf)), (0, 4, np.zeros((0, 4))), (3, 0, np.zeros((3, 4))), (3, 4, np.zeros((3, 0))),
                       (4097, 1, np.zeros((4097, 2))), (1, 1, np.zeros((1, 4098))), (True, 1, np.zeros((1, 4))), (3.0, 4, np.zeros((3, 4))),
                       (3, 4, 'taps')]:
        with pytest.raises(ValueError):
            sound.ResampleTable(L, M, taps)


@pytest.mark.parametrize('rate_in,rate_out,nsamp', TINY)
@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('dtype', [np.float32, np.int16])
def test_twin_is_the_double_loop(tables, rate_in, rate_out, nsamp, channels, dtype):
    x = ref.signal(nsamp, 10 * nsamp + channels, channels, dtype)
    L, M = ref.ratio(rate_in, rate_out)
    taps = tables.get((rate_in, rate_out))
    if taps is None:
        taps = ref.table(rate_in, rate_out)
    want = ref.direct(ref.mix(x), taps, L, M)
    got = sound.resample(x, rate_in, rate_out, device='cpu')
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert got.shape == want.shape == (sound.resampled_length(nsamp, rate_in, rate_out),) == (ref.length(nsamp, rate_in, rate_out),)
    assert np.array_equal(got, want)
    assert np.array_equal(ref.vectorised(ref.mix(x), taps, L, M), want)       # (the GPU tier's reference at the larger shapes)


def test_twin_with_a_custom_table_and_equal_rates():
    rs = np.random.RandomState(3)
    taps = rs.randn(3, 4)
    x = ref.signal(29, 4, 3)
    got = sound.resample(x, 4, 3, table=sound.ResampleTable(3, 4, taps), device='cpu')
    assert np.array_equal(got, ref.direct(ref.mix(x), taps, 3, 4))
    same = sound.resample(x, 16000, 16000, device='cpu')
    assert same.dtype == np.float32 and np.array_equal(same, ref.mix(x))
    i16 = ref.signal(9, 5, 2, np.int16)
    assert np.array_equal(sound.resample(i16, 7, 7, device='cpu'), ref.mix(i16))
    with pytest.raises(ValueError, match='L = 2 and M = 3'):
        sound.resample(x, 3, 2, table=sound.ResampleTable(3, 4, taps), device='cpu')
    with pytest.raises(ValueError):
        sound.resample(x, 4, 3, table=taps, device='cpu')
    for bad in (np.zeros((0,), np.float32), np.zeros((2, 2, 2), np.float32), np.zeros((4, 0), np.float32)):
        with pytest.raises(ValueError, match='waveform'):
            sound.resample(bad, 3, 2, device='cpu')


def test_lengths():
    for rate_in, rate_out in RATES + [(16000, 16000), (8000, 48000)]:
        for nsamp in (1, 2, 3, 440, 441, 442, 99999):
            want = ref.length(nsamp, rate_in, rate_out)
            assert sound.resampled_length(nsamp, rate_in, rate_out) == want
            assert (want - 1) * rate_in < nsamp * rate_out <= want * rate_in     # ceil(nsamp rate_out / rate_in)
    assert sound.resampled_length(3600 * 48000, 48000, 16000) == 3600 * 16000


@pytest.mark.parametrize('freq,passes', [(3000, True), (12000, False)])
def test_quality_of_the_definition(freq, passes):
    """44100 -> 16000 on 20000 samples of a float32 sine, away from 300 output samples at each end: 3000 Hz comes back within 1e-6
    of the analytic sine, 12000 Hz (above the new Nyquist frequency) is removed to below 1e-6.  Loose on purpose: the measured values
    are 2.3e-8 and 2.4e-8 (the float32 rounding of the input); a wrong cutoff, a missing gain c or a tap index off by one give 1e-2 or
    worse."""
    x, f = ref.sine(20000, freq, 44100)
    y = sound.resample(x, 44100, 16000, device='cpu').astype(np.float64)
    assert y.shape == (ref.length(20000, 44100, 16000),)
    want = f(np.arange(y.shape[0]) / 16000.0) if passes else np.zeros(y.shape[0])
    err = np.abs(y - want)[300:-300].max()
    print('%d Hz: largest deviation %.3e' % (freq, err))
    assert err <= 1e-6


def test_load_wav_round_trips(tmp_path):
    rs = np.random.RandomState(7)
    i16 = rs.randint(-32768, 32768, size=(50, 2)).astype(np.int16)
    f32 = (rs.rand(40) * 2 - 1).astype(np.float32)
    i32 = rs.randint(-2 ** 31, 2 ** 31, size=30, dtype=np.int64).astype(np.int32)
    u8 = rs.randint(0, 256, size=(20, 2)).astype(np.uint8)
    for name, rate, data, want in [('a.wav', 44100, i16, i16), ('b.wav', 16000, f32, f32),
                                   ('c.wav', 48000, i32, (i32 / 2.0 ** 31).astype(np.float32)),
                                   ('d.wav', 8000, u8, ((u8.astype(np.float64) - 128) / 128).astype(np.float32))]:
        path = str(tmp_path / name)
        wavfile.write(path, rate, data)
        got_rate, got = sound.load_wav(path)
        assert got_rate == rate and type(got_rate) is int and got.dtype == want.dtype and np.array_equal(got, want), name
    path = str(tmp_path / 'e.wav')
    wavfile.write(path, 16000, rs.rand(10))                                   # float64 samples
    with pytest.raises(ValueError, match='e.wav'):
        sound.load_wav(path)
    path = str(tmp_path / 'f.wav')
    with open(path, 'wb') as f:
        f.write(b'not a wav file at all')
    with pytest.raises(ValueError, match='f.wav'):
        sound.load_wav(path)
    with pytest.raises(ValueError, match='missing.wav'):
        sound.load_wav(str(tmp_path / 'missing.wav'))
    with pytest.raises(ValueError, match='f.wav'):
        pg.DeviceStripDataset.from_wav_files([path], frequency=16000, n_fft=16, hop_length=4, device='cpu')


def test_value_errors():
    y = np.zeros(4000, dtype=np.float32)
    with pytest.raises(ValueError, match='16001'):                             # L = 16001 phases
        sound.resample_table(44100, 16001)
    with pytest.raises(ValueError, match='at most'):
        sound.resample(y, 44100, 16001, device='cpu')
    with pytest.raises(ValueError, match='at most'):                           # T = 2 ceil(64 / (0.9476 / 31)) > 4096
        sound.resample_table(31, 1)
    for rate_in, rate_out in [(0, 16000), (-44100, 16000), (44100, 0), (44100.0, 16000), (44100, 16000.5), ('44100', 16000),
                              (True, 16000), (None, 16000)]:
        with pytest.raises(ValueError, match='positive integer'):
            sound.resample_table(rate_in, rate_out)
        with pytest.raises(ValueError, match='positive integer'):
            sound.resampled_length(100, rate_in, rate_out)
        with pytest.raises(ValueError, match='positive integer'):
            sound.resample(y, rate_in, rate_out, device='cpu')
    for kw in (dict(zeros=0), dict(rolloff=0.0), dict(rolloff=1.5), dict(beta=-1.0), dict(zeros=float('nan')), dict(beta='x')):
        with pytest.raises(ValueError, match='resample_table'):
            sound.resample_table(3, 2, **kw)
    # the sound ends: the checks come before anything touches a device
    for fn, arg in [(sound.spectrogram_u8, y), (sound.spectrogram_stack_u8, y[None]), (sound.spectrogram_strip_u8, y)]:
        with pytest.raises(ValueError, match='belong together'):
            fn(arg, 64, 16, rate_in=44100)
        with pytest.raises(ValueError, match='belong together'):
            fn(arg, 64, 16, frequency=16000)
        with pytest.raises(ValueError, match='positive integer'):
            fn(arg, 64, 16, rate_in=44100.0, frequency=16000)
        with pytest.raises(ValueError, match='sample_rate 22050'):
            fn(arg, 64, 16, img_mode='melif', sample_rate=22050, rate_in=44100, frequency=16000)
    with pytest.raises(ValueError, match="sample_rate and mel_rows belong to img_mode='melif'"):
        sound.spectrogram_strip_u8(y, 64, 16, img_mode='magif', sample_rate=16000, rate_in=44100, frequency=16000)
    # the strip dataset
    D = pg.DeviceStripDataset
    kw = dict(n_fft=16, hop_length=4, device='cpu')
    with pytest.raises(ValueError, match='rates: 2 values for 3 waveforms'):
        D.from_waveforms([y, y, y], rates=[44100, 16000], frequency=16000, **kw)
    with pytest.raises(ValueError, match='belong together'):
        D.from_waveforms([y], rates=44100, **kw)
    with pytest.raises(ValueError, match='belong together'):
        D.from_waveforms([y], frequency=16000, **kw)
    with pytest.raises(ValueError, match='positive integer'):
        D.from_waveforms([y, y], rates=[44100, 0], frequency=16000, **kw)
    with pytest.raises(ValueError, match='sample_rate 8000'):
        D.from_waveforms([y], rates=44100, frequency=16000, img_mode='melif', sample_rate=8000, **kw)
    # 80 samples at 44100 Hz are 30 at 16000 Hz: 7 usable frames every 4 samples, a window of n_fft/2 = 8 needs 8
    with pytest.raises(ValueError, match=r'waveform 0: 80 samples at 44100 Hz are 30 samples at 16000 Hz and give 7 usable frames, a window needs 8'):
        D.from_waveforms([y[:80], y], rates=44100, frequency=16000, **kw)


def test_binding_table_is_the_header():
    """Every prototype and #define of include/pggan_hip_resample.h lands in _lib.RESAMPLE_SIGNATURES / RESAMPLE_CONSTANTS, disjoint
    from every other table; the product header's counts (tests/test_abi_host.py) are not touched."""
    with open(os.path.join(ROOT, 'include', 'pggan_hip_resample.h')) as f:
        text = f.read()
    protos = re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', text)
    assert sorted(protos) == sorted(_lib.RESAMPLE_SIGNATURES) == ['pg_resample_mono']
    defines = dict(re.findall(r'^#define[ \t]+(PG_\w+)[ \t]+(\d+)[ \t]*$', text, flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == _lib.RESAMPLE_CONSTANTS == {
        'PG_RESAMPLE_F32': 0, 'PG_RESAMPLE_I16': 1, 'PG_RESAMPLE_MAX_PHASES': 4096, 'PG_RESAMPLE_MAX_TAPS': 4096}
    P, I, L = _lib.P, _lib.I, _lib.L
    assert _lib.RESAMPLE_SIGNATURES['pg_resample_mono'] == [P, I, L, I, P, I, I, I, P, L, P]
    others = (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.CLUSTER_SIGNATURES, _lib.GAN_SIGNATURES, _lib.PHASE_SIGNATURES,
              _lib.SAMPLING_SIGNATURES, _lib.PROJECTION_SIGNATURES, _lib.CROP_SIGNATURES, _lib.SWD_SIGNATURES, _lib.MEL_SIGNATURES)
    assert not any(set(_lib.RESAMPLE_SIGNATURES) & set(o) for o in others)
    assert not set(_lib.RESAMPLE_CONSTANTS) & set(_lib.CONSTANTS)
    assert _lib._RESTYPE_OF['pg_resample_mono'] is I
    assert (sound.RESAMPLE_MAX_PHASES, sound.RESAMPLE_MAX_TAPS) == (4096, 4096)
    assert '#include "pggan_hip_resample.h"' in open(os.path.join(ROOT, 'pggan-pytorch_amd', 'csrc', 'resample.hip')).read()
