"""The rate conversion on the device (include/pggan_hip_resample.h, csrc/resample.hip) against the numpy twin and the independent
restatement of tests/resample_ref.py.  Every comparison is ``==``: the kernel sums fp64 products in the definition's order."""
import numpy as np
import pytest
import torch
from scipy.io import wavfile

import resample_ref as ref

import pggan_amd as pg

pytestmark = pytest.mark.gpu
sound, _lib = pg.sound, pg._lib

# (rate_in, rate_out, nsamp): signals shorter than the filter (both edges inside one output's taps); L = 1 and M = 1; many phases,
# several workgroups and a ragged last run; tens of thousands of outputs
SHAPES = [(3, 2, 1), (3, 2, 5), (2, 3, 7), (5, 7, 33), (3, 1, 100), (1, 3, 50), (44100, 16000, 3000), (16000, 44100, 700),
          (3, 1, 210001)]
_tables = {}


def table(rate_in, rate_out):
    if (rate_in, rate_out) not in _tables:
        _tables[rate_in, rate_out] = ref.table(rate_in, rate_out)
    return _tables[rate_in, rate_out]


@pytest.mark.parametrize('rate_in,rate_out,nsamp', SHAPES)
def test_kernel_is_the_twin(rate_in, rate_out, nsamp):
    L, M = ref.ratio(rate_in, rate_out)
    for channels in (1, 2):
        for dtype in (np.float32, np.int16):
            x = ref.signal(nsamp, nsamp + 7 * channels, channels, dtype)
            want = ref.vectorised(ref.mix(x), table(rate_in, rate_out), L, M)        # == ref.direct (tests/test_resample_host.py)
            twin = sound.resample(x, rate_in, rate_out, device='cpu')
            got = sound.resample(x, rate_in, rate_out)
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (sound.resampled_length(nsamp, rate_in, rate_out),)
            got = got.cpu().numpy()
            assert np.array_equal(twin, want) and np.array_equal(got, want), (channels, dtype)
            again = sound.resample(torch.from_numpy(x).cuda(), rate_in, rate_out)      # a device tensor; the same bits twice
            assert np.array_equal(again.cpu().numpy(), want)


def test_custom_table():
    """The kernel knows no filter: random finite taps, L = 3, T = 4."""
    rs = np.random.RandomState(11)
    taps = rs.randn(3, 4)
    t = sound.ResampleTable(3, 4, taps)
    for nsamp, channels in [(1, 1), (2, 2), (1001, 3)]:
        x = ref.signal(nsamp, nsamp, channels)
        want = ref.direct(ref.mix(x), taps, 3, 4)
        assert np.array_equal(sound.resample(x, 4, 3, table=t, device='cpu'), want)
        assert np.array_equal(sound.resample(x, 4, 3, table=t).cpu().numpy(), want)
    # a ratio so large that a run of outputs is shorter than a workgroup, and more phases than a workgroup has threads
    for L, M, T, nsamp in [(1, 3000, 4, 20000), (300, 7, 6, 40)]:
        taps = rs.randn(L, T)
        x = ref.signal(nsamp, L, 1)
        got = sound.resample(x, M, L, table=sound.ResampleTable(L, M, taps))
        assert np.array_equal(got.cpu().numpy(), ref.vectorised(x, taps, L, M))


def test_equal_rates_are_the_mix_down():
    x = ref.signal(1000, 3, 2)
    got = sound.resample(x, 16000, 16000)
    assert torch.equal(got, torch.from_numpy(x).cuda().sum(dim=1) / 2) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), sound.resample(x, 16000, 16000, device='cpu'))
    mono = ref.signal(10, 4)
    assert np.array_equal(sound.resample(mono, 5, 5).cpu().numpy(), mono)
    i16 = ref.signal(100, 5, 2, np.int16)
    assert np.array_equal(sound.resample(i16, 44100, 44100).cpu().numpy(), ref.mix(i16))


def test_argument_errors_of_the_entry_point():
    C, RC = _lib.CONSTANTS, _lib.RESAMPLE_CONSTANTS
    fn = _lib.load().pg_resample_mono
    F32, I16 = RC['PG_RESAMPLE_F32'], RC['PG_RESAMPLE_I16']
    nsamp, L, M, T = 10, 2, 3, 4
    n_out = 7                                                                 # ceil(10 * 2 / 3)
    x = torch.zeros(nsamp * 2, device='cuda')
    taps = torch.zeros(8192 * 2 + 2, dtype=torch.float64, device='cuda')
    out = torch.zeros(16384, device='cuda')                                   # (room for the 13654 outputs of the widest call below)
    ok = dict(x=x.data_ptr(), fmt=F32, nsamp=nsamp, channels=2, taps=taps.data_ptr(), L=L, M=M, T=T, out=out.data_ptr(), n_out=n_out)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a['x'], a['fmt'], a['nsamp'], a['channels'], a['taps'], a['L'], a['M'], a['T'], a['out'], a['n_out'], None)

    assert call() == 0 and call(fmt=I16) == 0
    for kw in (dict(x=None), dict(taps=None), dict(out=None), dict(nsamp=0), dict(channels=0), dict(fmt=2), dict(fmt=-1), dict(L=0),
               dict(M=0), dict(T=3), dict(T=0), dict(T=1), dict(n_out=6), dict(n_out=8)):
        assert call(**kw) == C['PG_E_ARG'], kw
    for kw in (dict(x=x.data_ptr() + 4), dict(taps=taps.data_ptr() + 8), dict(out=out.data_ptr() + 4)):
        assert call(**kw) == C['PG_E_ALIGN'], kw
    assert call(L=4097, n_out=13657) == C['PG_E_UNSUP']                       # ceil(10 * 4097 / 3)
    assert call(T=4098) == C['PG_E_UNSUP']
    assert call(L=4096, n_out=13654, T=2) == 0 and call(L=1, M=1, n_out=10, T=4096) == 0      # the caps themselves are served
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        _lib.call('pg_resample_mono', x.data_ptr(), F32, nsamp, 2, taps.data_ptr(), L, M, T, out.data_ptr(), n_out + 1, None)


@pytest.fixture(scope='module')
def noise():
    """About one second at 44100 Hz, stereo, and its resampled mono form on the device."""
    y = ref.signal(44100, 21, 2) * np.float32(0.5)
    return y, sound.resample(y, 44100, 16000)


@pytest.mark.parametrize('img_mode', ['magif', 'abslog', 'melif'])
def test_strip_resamples_first(noise, img_mode):
    y, mono = noise
    got = sound.spectrogram_strip_u8(y, 64, 16, img_mode=img_mode, rate_in=44100, frequency=16000)
    want = sound.spectrogram_strip_u8(mono, 64, 16, img_mode=img_mode)
    assert tuple(got.shape) == (1 if img_mode == 'abslog' else 2, 32, 16000 // 16) and torch.equal(got, want)
    if img_mode == 'melif':                                                   # sample_rate follows the frequency
        assert torch.equal(got, sound.spectrogram_strip_u8(mono, 64, 16, img_mode='melif', sample_rate=16000))
        other = sound.spectrogram_strip_u8(y, 64, 16, img_mode='melif', rate_in=44100, frequency=22050)
        assert torch.equal(other, sound.spectrogram_strip_u8(sound.resample(y, 44100, 22050), 64, 16, img_mode='melif', sample_rate=22050))
    same = sound.spectrogram_strip_u8(mono, 64, 16, img_mode=img_mode, rate_in=16000, frequency=16000)   # equal rates: today's path
    assert torch.equal(same, want)


def test_image_and_stack_resample_first(noise):
    y, mono = noise
    for img_mode in ('abslog', 'magif'):
        got = sound.spectrogram_u8(y, 64, 16, img_mode=img_mode, rate_in=44100, frequency=16000)
        assert torch.equal(got, sound.spectrogram_u8(mono, 64, 16, img_mode=img_mode))
    rows = np.stack([y[:5000, 0], y[5000:10000, 1]])
    pre = torch.stack([sound.resample(r, 44100, 16000) for r in rows])
    for img_mode in ('magif', 'melif'):
        got = sound.spectrogram_stack_u8(rows, 64, 16, img_mode=img_mode, rate_in=44100, frequency=16000)
        assert tuple(got.shape) == (2, 2, 32, 32) and torch.equal(got, sound.spectrogram_stack_u8(pre, 64, 16, img_mode=img_mode))


def test_strip_dataset_from_waveforms_and_files(tmp_path):
    ys = [ref.signal(3000, 31, 2), ref.signal(900, 32), ref.signal(2500, 33, 2, np.int16)]
    rates = [44100, 16000, 48000]
    kw = dict(n_fft=16, hop_length=4, shuffle=False)
    ds = pg.DeviceStripDataset.from_waveforms(ys, rates=rates, frequency=16000, **kw)
    lengths = [sound.resampled_length(y.shape[0], r, 16000) for y, r in zip(ys, rates)]
    assert lengths == [1089, 900, 834] and ds.lengths == [8 * (n // 4 // 8) for n in lengths]
    pre = pg.DeviceStripDataset.from_waveforms([sound.resample(y, r, 16000) for y, r in zip(ys, rates)], **kw)
    assert pre.lengths == ds.lengths and len(ds) == len(pre)
    idx = torch.arange(len(ds), device='cuda')
    assert torch.equal(ds.items(idx), pre.items(idx))
    one = pg.DeviceStripDataset.from_waveforms(ys[:1], rates=44100, frequency=16000, **kw)       # one rate for all
    assert torch.equal(one.items(idx[:len(one)]), ds.items(idx[:len(one)]))
    # two files: int16 stereo at 44100 Hz and float32 mono at 16000 Hz
    a, b = ref.signal(3000, 41, 2, np.int16), ref.signal(1000, 42)
    pa, pb = str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav')
    wavfile.write(pa, 44100, a)
    wavfile.write(pb, 16000, b)
    files = pg.DeviceStripDataset.from_wav_files([pa, pb], frequency=16000, **kw)
    arrays = pg.DeviceStripDataset.from_waveforms([a, b], rates=[44100, 16000], frequency=16000, **kw)
    assert files.lengths == arrays.lengths == [8 * (1089 // 4 // 8), 8 * (1000 // 4 // 8)]
    idx = torch.arange(len(files), device='cuda')
    assert torch.equal(files.items(idx), arrays.items(idx))
