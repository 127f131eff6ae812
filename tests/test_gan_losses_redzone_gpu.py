"""The three kernels of csrc/gan_losses.hip between guard bands (tests/redzone.py, docs/experiments_redzone.md): scores, penalties and
image gradients are guarded inputs (NaN bands: a load from outside poisons a result), every output the wrappers allocate is a guarded
output filled with the sentinel.  No band is touched, no input is changed, every output element is written -- and the results are still
the reference's.  Payloads are 16-byte aligned and no better; E = 50 leaves rows that are not even that."""
import numpy as np
import pytest
import torch

import gan_losses_ref as ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    monkeypatch.setattr(ops, 'torch', r.proxy(helpers=(ops._empty, ops.Arena.take)))
    yield r
    r.forget()


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


def _inside(got, want, bound):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(-1)
    return bool(np.all(np.abs(got - np.asarray(want).reshape(-1)) <= np.broadcast_to(np.asarray(bound).reshape(-1), got.shape)))


@pytest.mark.parametrize('N', [1, 3, 65, 1000])
@pytest.mark.parametrize('kind', ref.KINDS)
def test_d_loss_between_guard_bands(rz, kind, N):
    for groups, with_pen in ((2, False), (3, True)):
        rs = np.random.RandomState(N + groups)
        s = (rs.randn(groups * N) * 3).astype(np.float32)
        pen = rs.rand(N).astype(np.float32) if with_pen else None
        s_d = rz.guard(torch.from_numpy(s), name='scores')
        pen_d = rz.guard(torch.from_numpy(pen), name='pen') if with_pen else None
        assert s_d.data_ptr() % 32 == 16
        got = ops.gan_d_loss(s_d, pen_d, N, kind, 0.001)
        chk(rz)                                                # one buffer of 1 + 2N floats and gscore of groups x N: every element written
        want = ref.gan_d_loss(s, pen, N, groups, kind, 0.001)
        assert all(_inside(a, *want[name]) for a, name in zip(got, ('d_cost', 'd_real', 'd_fake', 'gscore')))
        rz.forget()


@pytest.mark.parametrize('N', [1, 3, 65, 1000])
@pytest.mark.parametrize('kind', ref.KINDS)
def test_g_loss_between_guard_bands(rz, kind, N):
    s = (np.random.RandomState(N).randn(N) * 3).astype(np.float32)
    c, gs = ops.gan_g_loss(rz.guard(torch.from_numpy(s), name='scores'), kind)
    chk(rz)
    wc, ec, wg, eg = ref.gan_g_loss(s, kind)
    assert _inside(c, wc, ec) and _inside(gs, wg, eg)


@pytest.mark.parametrize('N,E', [(3, 16), (3, 50), (1, 1), (5, 1027), (4, 3072), (2, 3 * 1024 * 1024)])
def test_r1_seed_between_guard_bands(rz, N, E):
    """(3, 50): 150 floats, 37 float4 and a scalar tail of 2; (1, 1): the tail alone; (5, 1027): a tail of 3 behind more than one
    workgroup; (2, 3 x 1024^2): past the cap of the grid."""
    g = np.random.RandomState(N + E % 997).randn(N, E).astype(np.float32)
    ss = (g.astype(np.float64) ** 2).sum(1).astype(np.float32)
    g_d, ss_d = rz.guard(torch.from_numpy(g), name='g'), rz.guard(torch.from_numpy(ss), name='ss')
    pen, u = ops.r1_seed(g_d, ss_d, 10.0, 1.0 / N)
    chk(rz)
    wp, ep, wu, eu = ref.r1_seed(g, ss, 10.0, 1.0 / N)
    assert _inside(pen, wp, ep) and _inside(u, wu, eu)
