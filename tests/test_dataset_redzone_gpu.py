"""pg_real_batch_u8 between guard bands (tests/redzone.py, docs/experiments_redzone.md): the image stack, the indices and the
mirror flags are guarded inputs, the batch a guarded output filled with the sentinel.  The cases are the ones where the kernel's
8-byte loads and 16-byte stores could lean on more than the contract's 16-byte bases: three channels with side 4 and side 8
(planes at odd multiples of 16 and 64 bytes from a base that is 16 (mod 32)), five images, an index naming the stack's last image
(the last source byte is the payload's last byte) and a mirrored last image."""
import numpy as np
import pytest
import torch

from dataset_ref import make_stack
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops
M = 6


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


@pytest.mark.parametrize('C,S,dd', [(3, 4, 0), (3, 8, 0), (1, 8, 0), (3, 16, 0), (3, 8, 1), (3, 16, 1), (3, 16, 2), (1, 32, 2)])
@pytest.mark.parametrize('flags', ['mixed', 'null'])
def test_real_batch_inside_guard_bands(rz, C, S, dd, flags):
    stack = make_stack(M, C, S, seed=2)
    idx = np.array([M - 1, 0, 2, 2, M - 1])
    flip = np.array([0, 1, 0, 1, 1], dtype=np.uint8) if flags == 'mixed' else None
    stack_d, idx_d = rz.guard(torch.from_numpy(stack), name='stack'), rz.guard(torch.from_numpy(idx), name='idx')
    flip_d = rz.guard(torch.from_numpy(flip), name='flip') if flip is not None else None
    assert stack_d.data_ptr() % 32 == 16
    for alpha, range_out in ((0.3, (-1, 1)), (1.0, (0, 255))):
        got = ops.real_batch_u8(stack_d, idx_d, flip_d, dd, alpha, (0, 255), range_out)
        chk(rz)                                                # bands intact, inputs unchanged, every output element written
        assert got.data_ptr() % 32 == 16
        assert np.array_equal(got.cpu().numpy(), pg.dataset.batch_host(stack, idx, flip, dd, alpha, (0, 255), range_out))
