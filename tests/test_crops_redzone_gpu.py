"""pg_crop_batch_u8 between guard bands (tests/redzone.py, docs/experiments_redzone.md): the strip buffer, its table, the strip
indices, the start columns and the mirror flags are guarded inputs, the batch a guarded output filled with the sentinel.  The cases
are the ones where the kernel's aligned 8-byte loads around an unaligned window could lean outside the buffer: every legal start of
every strip, so a window that starts on the buffer's first payload byte, one that ends on its last (the last strip's pitch is its
column count), every odd start in between; three channels with 4 and 8 rows (planes at odd multiples of 16 bytes from a base
that is 16 (mod 32)); the byte-load path of the levels below 8x8 and of depthdiff > 0.  The padding bytes of the buffer hold 0xEE:
they may be read and must not reach a result."""
import numpy as np
import pytest
import torch

from crops_ref import all_starts, make_strips, windows
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops, StripLevel = pg.ops, pg.dataset.StripLevel


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    monkeypatch.setattr(ops, 'torch', r.proxy(helpers=(ops._empty, ops.Arena.take)))
    yield r
    r.forget()


def chk(rz):
    try:
        rz.check()
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


def host_level(strips):
    """The level's buffer and table on the host, padding bytes 0xEE."""
    C, S = strips[0].shape[:2]
    rows, total = StripLevel.layout(C, S, [s.shape[2] for s in strips])
    buf = np.full(total, 0xEE, dtype=np.uint8)
    for (off, pitch, cols), s in zip(rows, strips):
        buf[off:off + C * S * pitch].reshape(C, S, pitch)[:, :, :cols] = s
    return buf, np.array(rows, dtype=np.int64)


# the last strip has 16 or 48 columns: its rows have no padding, the last window ends on the last payload byte
@pytest.mark.parametrize('C,R,widths,dd', [(3, 4, (1, 3, 4), 0), (3, 8, (1, 3, 2), 0), (1, 8, (1, 3, 2), 0), (2, 16, (1, 2, 3), 0),
                                           (3, 16, (1, 2, 3), 0), (3, 4, (1, 3, 4), 1), (3, 8, (1, 3, 2), 1), (3, 16, (1, 2, 3), 2)])
@pytest.mark.parametrize('flags', ['mixed', 'null'])
def test_crop_batch_inside_guard_bands(rz, C, R, widths, dd, flags):
    strips = make_strips(C, R, widths=widths, seed=5)
    buf, table = host_level(strips)
    assert table[-1, 1] == table[-1, 2] and table[-1, 0] + C * R * table[-1, 1] == buf.size
    idx, u = all_starts(strips, R)
    assert (idx[0], u[0]) == (0, 0) and (idx[-1], u[-1]) == (len(strips) - 1, strips[-1].shape[2] - R) and np.any(u % 2 == 1)
    flip = (np.arange(idx.size) % 3 == 1).astype(np.uint8) if flags == 'mixed' else None
    level = StripLevel(rz.guard(torch.from_numpy(buf), name='strips'), rz.guard(torch.from_numpy(table), name='table'), C, R,
                       table[:, 2])
    idx_d, pos_d = rz.guard(torch.from_numpy(idx), name='idx'), rz.guard(torch.from_numpy(u), name='pos')
    flip_d = rz.guard(torch.from_numpy(flip), name='flip') if flip is not None else None
    assert level.buffer.data_ptr() % 32 == 16
    stack = windows(strips, idx, u, R)
    for alpha, range_out in ((0.3, (-1, 1)), (1.0, (0, 255))):
        got = ops.crop_batch_u8(level, idx_d, pos_d, flip_d, 0, dd, alpha, (0, 255), range_out)
        chk(rz)                                                # bands intact, inputs unchanged, every output element written
        assert got.data_ptr() % 32 == 16
        assert np.array_equal(got.cpu().numpy(), pg.dataset.batch_host(stack, np.arange(idx.size), flip, dd, alpha, (0, 255), range_out))
