"""Every entry point of include/pggan_hip_phase.h between guard bands (tests/redzone.py, docs/experiments_redzone.md) at its smallest
ragged shapes: n_fft 8 with 3 frames, batch 1 and 3, bins = n_fft/2 and n_fft/2 + 1; the 4 x 4 image for the spectrum (the wrapper's
smallest); the two-channel real batch at side 4 and 8.  Inputs are guarded with NaN bands (an outside load that reaches the result
poisons it and the comparison with tests/magif_ref.py fails), outputs are filled with the sentinel: no byte outside a tensor is read as
data or written, every output byte is written."""
import numpy as np
import pytest
import torch

import magif_ref as ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops, phase = pg.ops, pg.phase
BOUND = 1e-9


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    proxy = r.proxy(helpers=(ops._empty, ops.Arena.take))
    monkeypatch.setattr(ops, 'torch', proxy)
    monkeypatch.setattr(phase, 'torch', proxy)
    yield r
    r.forget()


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


def _signals(batch, ns=7):
    return np.stack([ref.signal(ns, 50 + b) for b in range(batch)])


@pytest.mark.parametrize('bins', [4, 5])
@pytest.mark.parametrize('batch', [1, 3])
def test_analysis_and_quantiser_inside_guard_bands(rz, batch, bins):
    n_fft, hop, frames = 8, 3, 3                               # 7 samples: 1 + 7 // 3 = 3 frames, the last one reflects at both ends
    y = _signals(batch)
    S, logmag, ifreq = (np.stack(a)[:, :bins, :frames] for a in zip(*[ref.analyse(s, n_fft, hop) for s in y]))
    y_d = rz.guard(torch.from_numpy(y), name='y')
    assert y_d.data_ptr() % 32 == 16
    lm, fr = phase.analyse(y_d, n_fft, hop, bins, frames)
    chk(rz)                                                    # bands intact, the input unchanged, every output element written
    M = np.abs(S).max()
    d = np.abs(fr.cpu().numpy() - ifreq)
    assert np.abs(lm.cpu().numpy() - logmag).max() <= BOUND * M and (np.minimum(d, 2 - d) * np.abs(S)).max() <= BOUND * M
    # the quantiser: a level may equal one sentinel byte, never both -- two runs, the outputs must agree with each other
    lm_d, fr_d = rz.guard(torch.from_numpy(logmag.copy()), name='logmag'), rz.guard(torch.from_numpy(ifreq.copy()), name='ifreq')
    outs = []
    for sentinel in (0, 1):
        out = rz.out((batch, 2, bins, frames), torch.uint8, name='image', sentinel=sentinel)
        pg._lib.call('pg_phase_quantise_u8', lm_d.data_ptr(), fr_d.data_ptr(), out.data_ptr(), batch, bins * frames, 0.0, 1.75, ops._stream())
        chk(rz, may_stay_unwritten=('image',))
        outs.append(out.cpu().numpy())
    want = np.stack([ref.quantise(logmag[b], ifreq[b], (0.0, 1.75)) for b in range(batch)])
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], want)
    got = phase.magif_u8(lm_d, fr_d, (0.0, 1.75))             # ... and through the wrapper's own allocation
    chk(rz, may_stay_unwritten=('magif_u8:0',))
    assert got.data_ptr() % 32 == 16 and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('batch', [1, 3])
def test_synthesis_inside_guard_bands(rz, batch):
    H = W = 4
    rs = np.random.RandomState(batch)
    img = ((rs.rand(batch, 2, H, W) * 2 - 1) * 1.25).astype(np.float32)
    spec_ref = np.stack([ref.spectrum(im) for im in img])      # [batch, H + 1, W]
    img_d = rz.guard(torch.from_numpy(img), name='img')
    spec, c = phase.spectrum(img_d, return_phase=True)
    chk(rz)
    assert np.abs(spec.cpu().numpy() - spec_ref.transpose(0, 2, 1)).max() <= BOUND * np.abs(spec_ref).max()
    assert np.abs(c.cpu().numpy() - np.stack([ref.running_sum(im, (-1, 1))[1] for im in img])).max() <= 1e-14
    # pieces at 3 frames: the spectrum's first three columns, guarded as the float64 pairs the entry point reads
    s3 = np.ascontiguousarray(spec_ref.transpose(0, 2, 1)[:, :3])
    s3_d = rz.guard(torch.view_as_real(torch.from_numpy(s3)), name='spec')
    got = phase.pieces(torch.view_as_complex(s3_d))
    chk(rz)
    want = np.stack([ref.pieces(s.T) for s in s3])
    assert tuple(got.shape) == (batch, 3, 8) and np.abs(got.cpu().numpy() - want).max() <= BOUND * np.abs(want).max()
    # the chain of the saver: spectrum, pieces, overlap-add (hop 3: 9 samples), normalise
    wave = ops.wave_normalize(phase.synthesise(img_d, 3), 2)
    chk(rz)                                                    # (the peak scratch of the normalisation included)
    want = np.stack([ref.synthesise(im, 3) for im in img])
    want = (want / np.abs(want).max(axis=1, keepdims=True)).repeat(2, axis=1)
    assert tuple(wave.shape) == (batch, 18) and np.abs(wave.cpu().numpy() - want).max() <= 1e-6


@pytest.mark.parametrize('S,dd', [(4, 0), (8, 0), (8, 1), (16, 0), (16, 2)])
def test_two_channel_real_batch_inside_guard_bands(rz, S, dd):
    rs = np.random.RandomState(S + dd)
    stack = rs.randint(0, 256, size=(6, 2, S, S)).astype(np.uint8)
    idx, flip = np.array([5, 0, 2, 2, 5]), np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    stack_d, idx_d = rz.guard(torch.from_numpy(stack), name='stack'), rz.guard(torch.from_numpy(idx), name='idx')
    flip_d = rz.guard(torch.from_numpy(flip), name='flip')
    for f_d, f, alpha, range_out in ((flip_d, flip, 0.3, (-1, 1)), (None, None, 1.0, (0, 255))):
        got = ops.real_batch_u8(stack_d, idx_d, f_d, dd, alpha, (0, 255), range_out)
        chk(rz)
        assert got.data_ptr() % 32 == 16 and tuple(got.shape) == (5, 2, S >> dd, S >> dd)
        assert np.array_equal(got.cpu().numpy(), pg.dataset.batch_host(stack, idx, f, dd, alpha, (0, 255), range_out))
