"""The entry point of csrc/kid.hip between guard bands (tests/redzone.py, docs/experiments_redzone.md) at ragged shapes: inputs 16-byte
aligned and no better, and the tile sums the wrapper allocates itself.  No band touched, inputs unchanged, every output element written
(the mirrored half of the self form included); rows past M and N are never loaded (the bands hold NaN: one load that reached a sum
would poison it); the results still meet tests/kid_ref.py."""
import numpy as np
import pytest
import torch

import kid_ref
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


def features(M, F, seed):
    return (np.random.RandomState(seed).randn(M, F) * 0.5 + 0.3).astype(np.float32)


def test_cross_form_inside_guard_bands(pg, rz):
    x, y = features(130, 48, 1), features(67, 48, 2)
    s = pg.ops.kid_tilesums_f64(rz.guard(torch.from_numpy(x), name='x'), rz.guard(torch.from_numpy(y), name='y'))
    chk(rz)
    want, bound = kid_ref.tilesums_exact(x, y)
    got = s.cpu().numpy()
    assert got.shape == (3, 2) and np.isfinite(got).all() and (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize('skip', [False, True])
def test_self_form_inside_guard_bands(pg, rz, skip):
    x = features(65, 16, 3)
    s = pg.ops.kid_tilesums_f64(rz.guard(torch.from_numpy(x), name='x'), skip_diagonal=skip)
    chk(rz)                                                    # sums[1][0], the mirror of a tile that is not computed, is written too
    want, bound = kid_ref.tilesums_exact(x, skip_diagonal=skip)
    got = s.cpu().numpy()
    assert got.shape == (2, 2) and np.isfinite(got).all() and (np.abs(got - want) <= bound).all() and np.array_equal(got, got.T)
