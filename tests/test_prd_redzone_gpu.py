"""Both entry points of csrc/prd.hip between guard bands (tests/redzone.py, docs/experiments_redzone.md): ragged image counts, a tail
in D, and the outputs the wrappers allocate themselves -- ``cand``, the k-th values of the second launch, counts and hits.  No band
touched, inputs unchanged, every output element written; the results still equal tests/prd_ref.py."""
import numpy as np
import pytest
import torch

import prd_ref
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


@pytest.mark.parametrize('N,k', [(129, 3), (5, 1), (129, 16)])
def test_kth_inside_guard_bands(pg, rz, N, k):
    """D = 48: three 16-byte pieces of a chunk, the other five are never loaded; 129 images: the second tile row and column hold one
    image and re-read it 127 times; 5 images: one ragged tile."""
    x = prd_ref.images(N, 3, 4, seed=41)
    xd = rz.guard(torch.from_numpy(x), name='x')
    assert xd.data_ptr() % 32 == 16
    got = pg.ops.prd_kth_u8(xd, k)
    chk(rz)                                                    # cand [N, blocks, k], values and indices of the top-k: all written
    assert got.cpu().tolist() == prd_ref.radii(x, k).tolist()


@pytest.mark.parametrize('Na,Nb', [(129, 5), (5, 129)])
@pytest.mark.parametrize('which', ['both', 'a', 'b'])
def test_ball_inside_guard_bands(pg, rz, Na, Nb, which):
    a, b = prd_ref.images(Na, 3, 4, seed=42), prd_ref.images(Nb, 3, 4, seed=43)
    dist = prd_ref.d2(a, b)
    rad_a = np.sort(dist, axis=1)[:, Nb // 2].copy() if which in ('both', 'a') else None
    rad_b = np.sort(dist, axis=0)[Na // 2].copy() if which in ('both', 'b') else None
    ad, bd = rz.guard(torch.from_numpy(a), name='a'), rz.guard(torch.from_numpy(b), name='b')
    rad_ad = rz.guard(torch.from_numpy(rad_a), name='rad_a') if rad_a is not None else None
    rad_bd = rz.guard(torch.from_numpy(rad_b), name='rad_b') if rad_b is not None else None
    got = pg.ops.prd_ball_u8(ad, bd, rad_ad, rad_bd)
    chk(rz)                                                    # the call zeroes what it writes: no count is left as the sentinel
    want = prd_ref.ball_counts(a, b, rad_a, rad_b)
    for g, w in zip(got, want):
        assert (g is None) == (w is None) and (g is None or g.cpu().tolist() == w)
