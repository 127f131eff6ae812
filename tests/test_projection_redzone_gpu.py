"""pg_pyr_loss_grad and one whole ``Projector.loss_and_grad`` pass between guard bands (tests/redzone.py, docs/experiments_redzone.md).
The images sit between NaN bands, 16-byte aligned and no better: a load from outside that reaches a result breaks the comparison with
tests/projection_ref.py.  Outputs are created through the allocator proxy, filled with the sentinel: no band is touched, no input
modified, every output element written.  The fp64 scratch is exempt from the last demand only (its contents mean nothing after the
call and the entry point does not use all of it at every size); its bands are checked like every other tensor's."""
import pytest
import torch

import projection_ref as ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops
U = 2.0 ** -23


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    proxy = r.proxy(helpers=(ops._empty, ops.Arena.take))
    monkeypatch.setattr(ops, 'torch', proxy)
    monkeypatch.setattr(pg.projection, 'torch', proxy)
    yield r
    r.forget()


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


@pytest.mark.parametrize('N,C,r', [(2, 3, 8), (1, 2, 128)])
def test_pyramid_loss_inside_guard_bands(rz, N, C, r):
    g = torch.Generator().manual_seed(r)
    img, tgt = torch.randn(N, C, r, r, generator=g), torch.randn(N, C, r, r, generator=g)
    weights = [1.0, 0.5] + [2.0] * (ref.levels(r) - 2)
    want_l, want_g = ref.pyramid_loss_ref(img, tgt, weights)
    bound_l, bound_g = ref.pyramid_bounds_ref(img, tgt, weights)
    img_d, tgt_d = rz.guard(img, name='img'), rz.guard(tgt, name='target')
    assert img_d.data_ptr() % 32 == 16 and tgt_d.data_ptr() % 32 == 16
    scratch = rz.out((ops.pyramid_scratch_words(N, C, r),), torch.float64, name='scratch')
    loss, grad = ops.pyramid_loss(img_d, tgt_d, weights, scratch=scratch)
    chk(rz, may_stay_unwritten=('scratch',), keep_outputs=True)          # loss and grad written in full, nothing outside them
    assert loss.data_ptr() % 32 == 16 and grad.data_ptr() % 32 == 16
    assert bool(((loss.cpu().double() - want_l).abs() <= U * bound_l).all())
    assert bool(((grad.cpu().double() - want_g).abs() <= U * bound_g).all())
    # the loss-only call: the same loss, and the gradient of the call before stays as it is (nothing but loss and scratch is written)
    kept = grad.clone()
    loss2, none = ops.pyramid_loss(img_d, tgt_d, weights, want_grad=False, scratch=scratch)
    chk(rz, may_stay_unwritten=('scratch',))
    assert none is None and torch.equal(loss2.cpu().view(torch.int32), loss.cpu().view(torch.int32))
    assert torch.equal(grad.view(torch.int32), kept.view(torch.int32))
    # without a scratch of the caller's the wrapper's own allocation is the exempt one
    loss3, _ = ops.pyramid_loss(img_d, tgt_d, weights, want_grad=False)
    chk(rz, may_stay_unwritten=('pyramid_loss:0',))
    assert torch.equal(loss3.cpu().view(torch.int32), loss.cpu().view(torch.int32))


def test_loss_and_grad_pass_inside_guard_bands(rz):
    """The whole pass: the forward pass's activations, the image, the loss block, the projector's packed weights and every hand-over of the
    sweep are allocations between bands."""
    torch.manual_seed(5)
    G = pg.Generator((1, 3, 16, 16), fmap_base=128, fmap_max=32, latent_size=32).to('cuda')        # 32, 32, 16 channels
    G.depth, G.alpha = 2, 0.5
    g = torch.Generator().manual_seed(6)
    z, targets = torch.randn(3, 32, generator=g), torch.rand(3, 3, 16, 16, generator=g) * 2 - 1
    z_d, t_d = rz.guard(z, name='z'), rz.guard(targets, name='targets')
    proj = pg.Projector(G)
    loss, dz = proj.loss_and_grad(z_d, t_d)
    chk(rz, may_stay_unwritten=(proj._scratch,))
    assert tuple(loss.shape) == (3,) and tuple(dz.shape) == (3, 32)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all()) and float(dz.abs().max()) > 0.0
    img = G.forward(z_d)
    want = ref.pyramid_loss_ref(img.cpu(), targets)[0]
    assert float((loss.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())      # (a second forward pass: atomics)
