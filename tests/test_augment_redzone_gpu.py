"""The kernels of csrc/augment.hip between guard bands (tests/redzone.py, docs/experiments_redzone.md): images in NaN bands, the table in
bands of its own, outputs pre-filled with the sentinel, at W = 4 (one 16-byte word per row: every neighbour word is outside the row) and
W = 16, under the extreme shifts and both flips.  No band touched, no input changed, every output element written; the results still
equal the numpy twin bit for bit -- a load from outside the source plane would bring a NaN (or a neighbouring image) into them."""
import numpy as np
import pytest
import torch

import augment_ref as ar
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


def _extreme_rows(H, W):
    """The shifts that reach furthest out of the plane in each direction, alone and together, with both flips; a cutout and a gain among them."""
    rows = [ar.row()]
    for flip in (0, 1):
        for dy, dx in ((0, W - 1), (0, 1 - W), (0, W), (0, -W), (H - 1, 0), (1 - H, 0), (H, 0), (-H, 0), (H - 1, W - 1), (1 - H, 1 - W),
                       (H - 1, 1 - W), (1 - H, W - 1), (1, 1), (-1, -3), (0, 2), (-1, W + 1), (1, -W - 3), (2 * H, 2 * W), (-2 * H, -2 * W)):
            rows.append(ar.row(flip=flip, dy=dy, dx=dx))
        rows.append(ar.row(flip=flip, dy=1, dx=-1, y0=0, y1=2, x0=W - 2, x1=W, gain=0.5))
        rows.append(ar.row(flip=flip, dx=2 ** 31 - 1, dy=-2 ** 31))            # any int32 is a valid entry
        rows.append(ar.row(flip=flip, dx=-2 ** 31, dy=2 ** 31 - 1, y0=-2 ** 31, y1=2 ** 31 - 1, x0=-5, x1=2))
    return np.asarray(rows, dtype=np.int32)


@pytest.mark.parametrize('W', [4, 16])
@pytest.mark.parametrize('C', [1, 3])
def test_gather_and_transpose_inside_guard_bands(pg, rz, C, W):
    H = W
    table = _extreme_rows(H, W)
    N = len(table)
    x = ar.images(N, C, H, W, seed=60 + W)
    xd, td = rz.guard(torch.from_numpy(x), name='x'), rz.guard(torch.from_numpy(table), name='table')
    assert xd.data_ptr() % 32 == 16 and td.data_ptr() % 32 == 16
    y = pg.ops.augment_apply(xd, td, 1)
    chk(rz)                                                    # the output the wrapper allocated: every element written
    assert np.array_equal(ar.bits(y.cpu().numpy()), ar.bits(pg.augment.apply_host(x, table, 1)))
    gx = pg.ops.augment_adjoint(xd, td)
    chk(rz)
    assert np.array_equal(ar.bits(gx.cpu().numpy()), ar.bits(pg.augment.adjoint_host(x, table)))
    # one image, one row of the table: the planes before and behind are the bands themselves
    for k in (1, 2, N - 1):
        x1, t1 = rz.guard(torch.from_numpy(x[k:k + 1]), name='x1'), rz.guard(torch.from_numpy(table[k:k + 1]), name='t1')
        y1, g1 = pg.ops.augment_apply(x1, t1, 1), pg.ops.augment_adjoint(x1, t1)
        chk(rz)
        assert np.array_equal(ar.bits(y1.cpu().numpy()), ar.bits(pg.augment.apply_host(x[k:k + 1], table[k:k + 1], 1)))
        assert np.array_equal(ar.bits(g1.cpu().numpy()), ar.bits(pg.augment.adjoint_host(x[k:k + 1], table[k:k + 1])))


@pytest.mark.parametrize('rows', [1, 5, 257])
def test_table_and_sign_count_inside_guard_bands(pg, rz, rows):
    U = pg.augment.uniform_host(3, 8, rows * 8).reshape(rows, 8)
    Ud = rz.guard(torch.from_numpy(U), name='U')
    got = pg.ops.augment_table(Ud, 16, 16, 0.25, 0.25, 0.5, 0.5, 0.5, True, 0.75)
    chk(rz)
    assert np.array_equal(got.cpu().numpy(), pg.augment.table_host(U, 16, 16, 0.25, 0.25, 0.5, 0.5, 0.5, True, 0.75))
    s = (U[:, 0] - np.float32(0.5)).astype(np.float32)
    sd = rz.guard(torch.from_numpy(s), name='scores')
    acc = rz.guard(torch.tensor([1.0, 2.0], dtype=torch.float64), kind='acc', name='acc')
    pg.ops.score_signs(sd, acc)
    chk(rz)
    assert acc.cpu().tolist() == [1.0 + float(np.sign(s).sum()), 2.0 + rows]
