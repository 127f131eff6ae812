"""The four entry points of csrc/embed.hip between guard bands (tests/redzone.py, docs/experiments_redzone.md), at the ragged shapes of
tests/test_fd_gpu.py: inputs 16-byte aligned and no better, and the outputs the wrappers allocate themselves -- the stem's map, the
pooled map, the features, mean, cov and the moments' scratch.  No band touched, inputs unchanged, every output element written (the
scratch included); the results still equal tests/fd_ref.py."""
import numpy as np
import pytest
import torch

import fd_ref
from redzone import Redzone

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


@pytest.fixture
def rz(pg, monkeypatch):
    r = Redzone('cuda')
    monkeypatch.setattr(pg.ops, 'torch', r.proxy(helpers=(pg.ops._empty, pg.ops.Arena.take)))
    yield r
    r.forget()


def chk(rz):
    try:
        rz.check()
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


def bits(shape, seed):
    return fd_ref.rne_bits(np.random.RandomState(seed).randn(*shape).astype(np.float32) * 1.5)


@pytest.mark.parametrize('C,r', [(1, 4), (3, 8), (4, 4)])
def test_stem_inside_guard_bands(pg, rz, C, r):
    x = np.random.RandomState(C + r).randint(0, 256, (3, C, r, r)).astype(np.uint8)
    xd = rz.guard(torch.from_numpy(x), name='x')
    assert xd.data_ptr() % 32 == 16
    y = pg.ops.emb_stem_u8_bf16(xd)
    chk(rz)                                                    # the zero channels are written too
    assert np.array_equal(fd_ref.bits_of_tensor(y), fd_ref.stem(x))


@pytest.mark.parametrize('shape', [(2, 8, 8, 16), (1, 4, 4, 8)])
def test_pool_inside_guard_bands(pg, rz, shape):
    b = bits(shape, 1)
    y = pg.ops.emb_pool2_bf16(rz.guard(fd_ref.tensor_of_bits(b), name='x'))
    chk(rz)
    assert np.array_equal(fd_ref.bits_of_tensor(y), fd_ref.pool2(b))


@pytest.mark.parametrize('shape', [(3, 4, 4, 128), (1, 4, 4, 8)])
def test_gap_inside_guard_bands(pg, rz, shape):
    b = bits(shape, 2)
    f = pg.ops.emb_gap_f32(rz.guard(fd_ref.tensor_of_bits(b), name='x'))
    chk(rz)
    assert np.array_equal(f.cpu().numpy(), fd_ref.gap(b))


@pytest.mark.parametrize('M,F', [(2, 16), (5, 16), (67, 48), (513, 128)])
def test_moments_inside_guard_bands(pg, rz, M, F):
    """Rows past M and columns past F are never loaded (the bands hold NaN: one load would poison the result); mean, cov and every value
    of the scratch -- column sums and tiles of every slice, the zero padding of a ragged tile included -- are written."""
    x = (np.random.RandomState(M + F).randn(M, F) + 3.0).astype(np.float32)
    mean, cov = pg.ops.fd_moments_f64(rz.guard(torch.from_numpy(x), name='x'))
    chk(rz)
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    want, mag = fd_ref.cov_exact(x, mean)
    assert np.isfinite(mean).all() and np.isfinite(cov).all() and np.array_equal(cov, cov.T)
    assert (np.abs(mean - fd_ref.mean_exact(x)) <= (M + 1) * 2.0 ** -53 * np.abs(x.astype(np.float64)).sum(axis=0) / M).all()
    assert (np.abs(cov - want) <= 2 * (M + 4) * 2.0 ** -53 * mag / (M - 1)).all()
