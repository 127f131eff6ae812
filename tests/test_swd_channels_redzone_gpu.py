"""Every entry point of include/pggan_hip_swd.h between guard bands (tests/redzone.py, docs/experiments_redzone.md) for 1, 2 and 4
channels at ragged shapes: a gather into the middle of a larger buffer, the statistics and the normalisation of 37 and 1000
descriptors (one workgroup and several of the two-stage reduction), and the projection with a ragged last workgroup (37 and
1000 = 7 x 128 + 104 rows) against one direction and against a full block plus a partial one (160).  The projection of four
channels pads its rows in LDS; the descriptors in memory are 196 floats apart and nothing behind the last one may be read."""
import pytest
import torch

import swd_ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops
# pg_swd_channel_stats_c: "partials: PG_SWD_REDUCE_BLOCKS * 2 C doubles of scratch" -- scratch, as many as the launch has workgroups
SWD_PARTIALS = ('_swd_partials:0',)


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


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('C', [1, 2, 4])
def test_gather_inside_guard_bands(rz, C):
    S, N, P, off = 16, 3, 5, 4
    level = torch.randn(N, C, S, S, generator=gen(S + C))
    centres = torch.randint(3, S - 3, (N * P, 2), generator=gen(S + 1), dtype=torch.int32)
    centres[0], centres[4], centres[7], centres[14] = torch.tensor([[3, 3], [S - 4, 3], [3, S - 4], [S - 4, S - 4]], dtype=torch.int32)
    rows = off + N * P + 3
    out = rz.guard(torch.full((rows, 49 * C), -7.5), inplace=True, name='descriptors')
    ops.swd_gather_c(rz.guard(level), rz.guard(centres), P, out, off)
    chk(rz)
    assert torch.equal(out[off:off + N * P].cpu(), swd_ref.descriptors(level, centres, P).reshape(N * P, 49 * C))
    assert bool((out[:off] == -7.5).all()) and bool((out[off + N * P:] == -7.5).all())
    # the last image's last rows, written up to the buffer's last float
    tight = rz.guard(torch.full((N * P, 49 * C), -7.5), inplace=True, name='descriptors, no spare rows')
    ops.swd_gather_c(rz.guard(level), rz.guard(centres), P, tight, 0)
    chk(rz)
    assert torch.equal(tight.cpu(), swd_ref.descriptors(level, centres, P).reshape(N * P, 49 * C))


@pytest.mark.parametrize('M', [37, 1000])
@pytest.mark.parametrize('C', [1, 2, 4])
def test_stats_and_normalise_inside_guard_bands(rz, C, M):
    scale, mean = torch.tensor([0.5, 2.0, 1.0, 3.0][:C]).view(1, C, 1, 1), torch.tensor([3.0, -1.0, 0.1, -4.0][:C]).view(1, C, 1, 1)
    desc = torch.randn(M, C, 7, 7, generator=gen(M + C)) * scale + mean
    d = rz.guard(desc.reshape(M, 49 * C).contiguous(), inplace=True)
    ops.swd_normalize_c_(d)
    chk(rz, may_stay_unwritten=SWD_PARTIALS)                   # (the [2 C] statistics must be written whole)
    assert float((d.cpu().double() - swd_ref.normalize(desc.double())).abs().max()) <= 1e-5


@pytest.mark.parametrize('K', [1, 160])
@pytest.mark.parametrize('M', [37, 1000])
@pytest.mark.parametrize('C', [1, 2, 4])
def test_project_inside_guard_bands(rz, C, M, K):
    W = 49 * C
    desc = torch.randn(M, W, generator=gen(1000 * M + K + C))
    dirs = torch.randn(W, K, generator=gen(K + C), dtype=torch.float64)
    dirs = (dirs / dirs.pow(2).sum(dim=0, keepdim=True).sqrt()).float().contiguous()
    got = ops.swd_project_c(rz.guard(desc), rz.guard(dirs))
    chk(rz)                                                    # bands intact, inputs unchanged, every element of [K,M] written
    assert tuple(got.shape) == (K, M)
    err = float((got.cpu().double() - (desc.double() @ dirs.double()).t()).abs().max())
    assert err <= (2e-5 if W <= 147 else 2e-5 * 196 / 147)
