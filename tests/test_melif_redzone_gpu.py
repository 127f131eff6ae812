"""Both entry points of include/pggan_hip_mel.h between guard bands (tests/redzone.py, docs/experiments_redzone.md) at their smallest
ragged shapes, patterned on tests/test_magif_redzone_gpu.py: the analysis at n_fft 8 with 4 rows from 7 samples every 3 (3 frames, the
last one reflects at both ends), batch 1 and 2, and at n_fft 16 with 4 rows (bands of several bins); the spectrum at M = W = 4 from
H = 4 and H = 8 bins.  The six arrays of the table sit between bands too (integer bands read as large positive numbers: an index taken
from one would point far outside).  Inputs are guarded with NaN bands (an outside load that reaches the result poisons it and the
comparison with tests/melif_ref.py fails), outputs are filled with the sentinel: no byte outside a tensor is read as data or written,
every output byte is written."""
import numpy as np
import pytest
import torch

import melif_ref as ref
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


def guarded_table(rz, tab):
    """The reference's table as a phase.MelTable whose device arrays lie between guard bands."""
    t = pg.MelTable(tab.n_fft, *tab.arrays())
    names = ('start', 'count', 'offset', 'weights', 'lower', 'frac')
    arrays = (t.start, t.count, t.offset, t.weights, t.lower, t.frac)
    t._on[torch.device('cuda', torch.cuda.current_device())] = tuple(rz.guard(torch.from_numpy(np.array(a)), name='table.' + n)
                                                                     for n, a in zip(names, arrays))
    return t


@pytest.mark.parametrize('n_fft,batch', [(8, 1), (8, 2), (16, 1)])
def test_analysis_inside_guard_bands(rz, n_fft, batch):
    M, hop = 4, 3
    ns = 7 if n_fft == 8 else 9                                # 7 samples: 3 frames; n_fft 16 pads by 8 and needs more than 8: 9 samples, 4 frames
    frames = 1 + ns // hop
    y = np.stack([ref.signal(ns, 50 + b) for b in range(batch)])
    tab = ref.table(n_fft, M)
    _, logmag, g, z = (np.stack(a) for a in zip(*[ref.analyse(s, n_fft, hop, tab) for s in y]))
    t = guarded_table(rz, tab)
    y_d = rz.guard(torch.from_numpy(y), name='y')
    assert y_d.data_ptr() % 32 == 16
    lm, fr = phase.mel_analyse(y_d, n_fft, hop, t)
    chk(rz)                                                    # bands intact, the inputs unchanged, every output element written
    assert tuple(lm.shape) == tuple(fr.shape) == (batch, M, frames) and lm.data_ptr() % 32 == 16
    dist = np.abs(ref.wrap(fr.cpu().numpy() - g)) * np.abs(z)
    assert np.abs(lm.cpu().numpy() - logmag).max() <= BOUND * logmag.max() and dist.max() <= BOUND * np.abs(z).max()
    # fewer frames than there are: the planes are smaller, nothing is written past them
    lm2, fr2 = phase.mel_analyse(y_d, n_fft, hop, t, frames=2)
    chk(rz)
    assert torch.equal(lm2, lm[:, :, :2]) and torch.equal(fr2, fr[:, :, :2])
    # ... and the quantiser behind it, through the public chain (its own guard-band test is tests/test_magif_redzone_gpu.py)
    img = phase.mel_spectrogram_stack_u8(y_d, n_fft, hop, t, frames=frames)
    chk(rz, may_stay_unwritten=('magif_u8:0',))               # (a level may equal the sentinel byte)
    want = np.stack([ref.image(s, n_fft, hop, tab, frames=frames)[0] for s in y])
    assert np.array_equal(img.cpu().numpy(), want)


@pytest.mark.parametrize('H', [4, 8])
@pytest.mark.parametrize('batch', [1, 3])
def test_synthesis_inside_guard_bands(rz, batch, H):
    M = W = 4
    rs = np.random.RandomState(batch + H)
    img = ((rs.rand(batch, 2, M, W) * 2 - 1) * 1.25).astype(np.float32)
    tab = ref.table(2 * H, M)
    spec_ref, c_ref = (np.stack(a) for a in zip(*[ref.spectrum(im, tab) for im in img]))       # [batch, H + 1, W], [batch, H, W]
    t = guarded_table(rz, tab)
    img_d = rz.guard(torch.from_numpy(img), name='img')
    spec, c = phase.mel_spectrum(img_d, t, return_phase=True)
    chk(rz)
    assert tuple(spec.shape) == (batch, W, H + 1) and tuple(c.shape) == (batch, H, W)
    assert np.abs(spec.cpu().numpy() - spec_ref.transpose(0, 2, 1)).max() <= BOUND * np.abs(spec_ref).max()
    assert np.abs(c.cpu().numpy() - c_ref).max() <= 1e-14
    plain = phase.mel_spectrum(img_d, t)                       # csum == NULL
    chk(rz)
    assert torch.equal(torch.view_as_real(plain), torch.view_as_real(spec))
    # the chain of the saver: spectrum, pieces, overlap-add (hop 3: 9 samples), normalise
    wave = ops.wave_normalize(phase.mel_synthesise(img_d, 3, t), 2)
    chk(rz)                                                    # (the peak scratch of the normalisation included)
    want = np.stack([ref.synthesise(im, 3, tab) for im in img])
    want = (want / np.abs(want).max(axis=1, keepdims=True)).repeat(2, axis=1)
    assert tuple(wave.shape) == (batch, 18) and np.abs(wave.cpu().numpy() - want).max() <= 1e-6
