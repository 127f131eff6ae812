"""Guard bands (tests/redzone.py) around everything pg_shift_l2min_u8 is handed: the level buffer, the strip table, the segment table,
the queries and the keys.  The buffer is 16-byte aligned and no better, and its last strip ends at the payload's last byte, so a read
past a strip's last row lands in the tail band (0x7F bytes) and a result that used it differs from the reference; a store outside the
keys, or a key that is never written, is reported by ``Redzone.check``.  S = 4 is the plain integer kernel, S = 32 the MFMA kernel; a
strip with T = S (one start) sits in the middle and at the very end of the buffer; K = 1 and K = 65 (two passes, the second into the
last row of the keys)."""
import numpy as np
import pytest
import torch

import shiftnn_ref
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


@pytest.mark.parametrize('S', [4, 32])
@pytest.mark.parametrize('K', [1, 65])
@pytest.mark.parametrize('seg', [None, 3])
def test_shift_l2min_inside_guard_bands(pg, rz, S, K, seg):
    C = 2
    cols = [S + 21, S, S + 140, S]                             # one start in the middle; two workgroups; one start at the end of the buffer
    strips = shiftnn_ref.strips(cols, C, S, seed=40 + S)
    q = shiftnn_ref.queries(K, C, S, seed=41 + S)
    host = pg.dataset.StripLevel.pack(strips, 'cpu')
    level = pg.dataset.StripLevel(rz.guard(host.buffer, name='level buffer'), rz.guard(host.table, name='strip table'), C, S, cols)
    assert level.buffer.data_ptr() % 32 == 16
    first = pg.ops.shift_segments(cols, S, seg)[2].tolist()
    tiles = np.concatenate([[0], np.cumsum([-(-(c - S + 1) // pg.ops.SHIFT_TILE) for c in cols])]).tolist()
    segtab = rz.guard(torch.tensor(list(zip(first, tiles)), dtype=torch.int64), name='segment table')
    queries = rz.guard(torch.from_numpy(q), name='queries')
    got = pg.ops.shift_l2min_u8(level, queries, seg, table=segtab)
    chk(rz)                                                    # bands intact, inputs unchanged, every key written
    assert np.array_equal(got.cpu().numpy(), shiftnn_ref.keys(strips, q, S if seg is None else seg))
