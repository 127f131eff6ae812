"""Magnitude + instantaneous frequency on the host: the definitions of tests/magif_ref.py against themselves,
``sound.SoundSaver(mode='magif')`` (the product's host twin) against them, the argument checks and the binding tables of
include/pggan_hip_phase.h.  No GPU.

"The test signal" of this file and of tests/test_magif_gpu.py is ``magif_ref.signal(ns, seed)``: with t = arange(ns),
clip(0.5 sin(2 pi (0.01 t + 0.2 t^2 / (2 ns))) + 0.1 RandomState(seed).randn(ns), -1, 1) as float32.

Every comparison prints its measured maximum before it asserts (docs/experiments_magif.md)."""
import ctypes
import os
import re

import numpy as np
import pytest

import magif_ref as ref
import pggan_amd as pg
from oracle import sound_steps as oss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9                                                               # the project's bound between independent fp64 transforms


@pytest.mark.parametrize('n_fft,hop', [(64, 16), (1024, 256)])
def test_definitions_invert_each_other(n_fft, hop):
    """Reference analysis with all n_fft/2 + 1 bins, then reference synthesis: the waveform again on the interior (hop = n_fft/4 is the
    exact-inverse regime of the 2/3 gain; the ends lack their overlapping frames)."""
    ns = 12 * n_fft
    y = ref.signal(ns, n_fft)
    _, logmag, ifreq = ref.analyse(y, n_fft, hop)
    assert logmag.shape == ifreq.shape == (n_fft // 2 + 1, 1 + ns // hop)
    assert ifreq.min() >= -1.0 and ifreq.max() < 1.0
    x = ref.from_planes(logmag, ifreq, hop)
    err = float(np.abs(x[n_fft:ns - n_fft] - y.astype(np.float64)[n_fft:ns - n_fft]).max())
    print('round trip n_fft=%d hop=%d: max|diff| on the interior %.3e' % (n_fft, hop, err))
    assert x.shape == (ns,) and err <= BOUND


def test_first_column_is_the_phase_and_rows_sum_to_it():
    y = ref.signal(700, 3)
    S, _, ifreq = ref.analyse(y, 32, 8)
    phi = np.arctan2(S.imag, S.real) / np.pi
    assert np.array_equal(ifreq[:, 0], ref.wrap(phi[:, 0]))
    back = ref.wrap(np.cumsum(ifreq, axis=1) - phi)
    print('running sum minus the phase, modulo 2: max %.3e' % np.abs(back).max())
    assert np.abs(back).max() <= 1e-12


def test_quantiser_landmarks():
    """IF 0, +-1/2 and -1 on levels 128, 192 / 64 and 0; a value that rounds to 256 is level 0; ties go to the even level."""
    f = np.array([0.0, 0.5, -0.5, -1.0, 1.0 - 2.0 ** -53, 1.0 / 256, 3.0 / 256, -1.0 / 256])
    assert (f[4] + 1.0) * 128 == 256.0
    for q in (ref.quantise, pg.sound.magif_image):
        img = q(np.zeros_like(f), f, (0.0, 1.0))
        assert img.dtype == np.uint8 and img[1].tolist() == [128, 192, 64, 0, 0, 128, 130, 128], q
    m = np.array([-0.1, 0.0, 0.4 / 255, 1.6 / 255, 1.0, 1.1, 100.0 / 255])
    for q in (ref.quantise, pg.sound.magif_image):
        assert q(m, np.zeros_like(m), (0.0, 1.0))[0].tolist() == [0, 0, 0, 2, 255, 255, 100], q
    # the default range is never clipped for |y| <= 1: |S| <= sum(window) = n_fft/2
    assert abs(oss.hann_periodic(64).sum() - 32.0) < 1e-12 and ref.default_mag_range(64) == (0.0, float(np.log1p(32)))
    assert pg.phase.default_mag_range(64) == ref.default_mag_range(64)


@pytest.mark.parametrize('n_fft,hop', [(16, 3), (64, 16)])
def test_host_analysis_and_image_match_the_reference(n_fft, hop):
    y = ref.signal(40 * n_fft, 7)
    S, logmag, ifreq = ref.analyse(y, n_fft, hop)
    lm, fr = pg.sound.magif_analyse(y, n_fft, hop)
    M = float(np.abs(S).max())
    d = np.abs(fr - ifreq)
    dist = np.minimum(d, 2 - d) * np.abs(S)
    print('host analysis n_fft=%d: |dlogmag| %.3e, weighted IF distance %.3e, max|S| %.3e' % (n_fft, np.abs(lm - logmag).max(), dist.max(), M))
    assert np.abs(lm - logmag).max() <= BOUND * M and dist.max() <= BOUND * M
    h = n_fft // 2
    a, b = pg.sound.magif_image(lm[:h, :h], fr[:h, :h], ref.default_mag_range(n_fft)), ref.image(y, n_fft, hop)
    print('host image n_fft=%d: %d of %d pixels differ' % (n_fft, int((a != b).sum()), a.size))
    assert a.shape == b.shape == (2, h, h) and np.array_equal(a, b)


@pytest.mark.parametrize('H,hop,scale', [(16, 8, 1.0), (32, 8, 1.5)])
def test_host_saver_equals_the_reference(H, hop, scale, tmp_path):
    from scipy.io import wavfile
    rs = np.random.RandomState(H)
    out = ((rs.rand(2, 2, H, H) * 2 - 1) * scale).astype(np.float32)
    saver = pg.SoundSaver(str(tmp_path), resolution=2 * H, hop_length=hop, mode='magif', seed=5)
    state = saver._rng.get_state()
    for i in range(2):
        want = ref.synthesise(out[i], hop)
        got = saver.image_to_sound(out[i])
        err = float(np.abs(got - want / np.abs(want).max()).max())
        print('host saver H=%d sample %d: max|diff| %.3e of a peak of 1' % (H, i, err))
        assert got.shape == want.shape == ((H - 1) * hop,) and err <= BOUND
    saver(out, 3)
    assert sorted(os.listdir(str(tmp_path))) == ['fakes_sound_000003_00.wav', 'fakes_sound_000003_01.wav']
    sr, wav = wavfile.read(str(tmp_path / 'fakes_sound_000003_01.wav'))
    want = ref.synthesise(out[1], hop)
    assert sr == 16000 and wav.dtype == np.float32 and np.abs(wav - (want / np.abs(want).max()).repeat(2)).max() < 1e-5
    assert all(np.array_equal(a, b) for a, b in zip(state, saver._rng.get_state()))       # no random start: the RNG is not advanced
    # an explicit range is used
    wide = pg.SoundSaver(create_subdirs=False, hop_length=hop, mode='magif', mag_range=(0.0, 2.0))
    want = ref.synthesise(out[0], hop, mag_range=(0.0, 2.0))
    assert np.abs(wide.image_to_sound(out[0]) - want / np.abs(want).max()).max() <= BOUND


def test_arguments():
    y = ref.signal(600, 1)
    with pytest.raises(ValueError, match='img_mode'):
        pg.spectrogram_u8(y, 64, 16, img_mode='ifmag')
    with pytest.raises(ValueError, match='mag_range'):
        pg.spectrogram_u8(y, 64, 16, img_mode='abslog', mag_range=(0, 1))
    for bad in ((1.0, 1.0), (2.0, 1.0), (0.0, float('nan')), (0.0, float('inf')), 3.0, (0.0, 1.0, 2.0), 'ab'):
        with pytest.raises(ValueError, match='mag_range'):
            pg.phase.check_mag_range(bad, 64, 'f')
        with pytest.raises(ValueError, match='mag_range'):
            pg.SoundSaver(create_subdirs=False, mode='magif', mag_range=bad)
    with pytest.raises(ValueError, match='mag_range'):
        pg.SoundSaver(create_subdirs=False, mode='abslog', mag_range=(0.0, 1.0))
    assert pg.phase.check_mag_range(None, 64, 'f') == ref.default_mag_range(64) and pg.phase.check_mag_range([0, 2], 64, 'f') == (0.0, 2.0)
    with pytest.raises(ValueError, match='two-channel'):
        pg.SoundSaver(create_subdirs=False, mode='magif').image_to_sound(np.zeros((16, 16), np.float32))
    with pytest.raises(ValueError, match='two-channel'):
        pg.SoundSaver(create_subdirs=False, mode='magif').image_to_sound(np.zeros((3, 16, 16), np.float32))
    with pytest.raises(ValueError):
        pg.SoundSaver(create_subdirs=False, mode='ifmag').image_to_sound(np.zeros((2, 16, 16), np.float32))
    with pytest.raises(ValueError, match='signals'):
        pg.spectrogram_stack_u8(y, 64, 16)                                  # [nsamp], not [batch, nsamp]
    with pytest.raises(ValueError, match='n_fft'):
        pg.spectrogram_stack_u8(y[None], 64.5, 16)
    import torch
    for bad in (torch.zeros(2, 1, 16, 16), torch.zeros(2, 2, 16, 16, dtype=torch.float64)):   # host tensors never reach a kernel
        with pytest.raises(ValueError, match='images'):
            pg.phase.spectrum(bad)
    with pytest.raises(ValueError, match='signals'):
        pg.phase.analyse(torch.zeros(2, 100), 64, 16)
    with pytest.raises(ValueError, match='logmag'):
        pg.phase.magif_u8(torch.zeros(1, 4, 4, dtype=torch.float64), torch.zeros(1, 4, 4, dtype=torch.float64), (0.0, 1.0))
    with pytest.raises(ValueError, match='spec'):
        pg.phase.pieces(torch.zeros(1, 4, 5, dtype=torch.complex128))
    # two channels: the dataset takes them, the metrics that are defined for 1 or 3 keep refusing
    ds = pg.DeviceImageDataset(np.zeros((3, 2, 8, 8), np.uint8), device='cpu', two_channel=True)
    assert ds.shape == (3, 2, 8, 8) and tuple(ds.batch(2).shape) == (2, 2, 4, 4)
    with pytest.raises(ValueError, match='channels'):
        pg.DeviceImageDataset(np.zeros((3, 4, 8, 8), np.uint8), device='cpu', two_channel=True)
    with pytest.raises(ValueError, match='two_channel'):
        pg.DeviceImageDataset(np.zeros((3, 2, 8, 8), np.uint8), device='cpu')        # unannounced: a sliced RGB stack, as before
    with pytest.raises(ValueError):
        pg.metrics.SlicedWasserstein(16, 64, num_channels=2)
    with pytest.raises(ValueError):
        pg.metrics.MultiScaleSSIM(16, 4, num_channels=2)


def test_two_channel_host_batches_are_the_per_channel_batches():
    """Host mode of DeviceImageDataset at C = 2: every plane of a batch is the plane a one-channel dataset of that channel gives."""
    rs = np.random.RandomState(2)
    stack = rs.randint(0, 256, size=(5, 2, 16, 16)).astype(np.uint8)
    for pyramid in ('chain', 'direct'):
        for depth, alpha in ((2, 1.0), (1, 0.5), (0, 0.5)):
            kw = dict(model_initial_depth=depth, alpha=alpha, pyramid=pyramid, mirror_augment=True, seed=4, device='cpu')
            both = pg.DeviceImageDataset(stack, two_channel=True, **kw).batch(7).numpy()
            for c in range(2):
                one = pg.DeviceImageDataset(stack[:, c:c + 1].copy(), **kw).batch(7).numpy()
                assert np.array_equal(both[:, c:c + 1], one), (pyramid, depth, alpha, c)


def test_phase_header_parses_completely():
    """Every prototype of include/pggan_hip_phase.h lands in _lib.PHASE_SIGNATURES and every #define in PHASE_CONSTANTS; the product
    header's tables are not touched by the addition; the built library exports each of them."""
    _lib = pg._lib
    with open(os.path.join(ROOT, 'include', 'pggan_hip_phase.h')) as f:
        text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', f.read(), flags=re.S)
    protos = re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', text)
    assert sorted(protos) == sorted(_lib.PHASE_SIGNATURES) == ['pg_phase_analyse_f64', 'pg_phase_pieces_f64', 'pg_phase_quantise_u8',
                                                               'pg_phase_spectrum_f64', 'pg_real_batch_2ch_u8']
    defines = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(PG_\w+)[ \t]+(\S+)[ \t]*$', text, flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == _lib.PHASE_CONSTANTS == dict(PG_PHASE_MIN_N=8, PG_PHASE_MAX_N=2048,
                                                                                    PG_PHASE_IF_LEVELS=256, PG_PHASE_IF_ZERO=128)
    P, I, L, D = _lib.P, _lib.I, _lib.L, _lib.D
    assert _lib.PHASE_SIGNATURES['pg_phase_analyse_f64'] == [P, L, I, P, P, I, I, I, I, P]
    assert _lib.PHASE_SIGNATURES['pg_phase_quantise_u8'] == [P, P, P, I, L, D, D, P]
    assert _lib.PHASE_SIGNATURES['pg_phase_spectrum_f64'] == [P, P, P, I, I, I, D, D, D, D, D, D, P]
    assert _lib.PHASE_SIGNATURES['pg_phase_pieces_f64'] == [P, P, I, I, I, P]
    assert _lib.PHASE_SIGNATURES['pg_real_batch_2ch_u8'] == [P, L, I, I, P, P, I, P, D, D, D, D, D, P]
    assert not set(_lib.PHASE_SIGNATURES) & set(_lib.SIGNATURES) and not set(_lib.PHASE_CONSTANTS) & set(_lib.CONSTANTS)
    assert len(_lib.SIGNATURES) == 96 and len(_lib.CONSTANTS) == 27 and _lib.ABI_VERSION == 27
    assert (pg.phase.MIN_N, pg.phase.MAX_N, pg.phase.IF_LEVELS, pg.phase.IF_ZERO) == (8, 2048, 256, 128)
    src = open(os.path.join(ROOT, 'pggan-pytorch_amd', 'phase.py')).read()
    assert set(re.findall(r"_C\['(PG_\w+)'\]", src)) == set(_lib.PHASE_CONSTANTS)
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    for name in protos:
        assert hasattr(lib, name), name
