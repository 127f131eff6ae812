"""pg_real_batch_u8 (csrc/real_batch.hip) and DeviceImageDataset on the MI355X against host mode, the oracle and the reference's own
outputs (tests/golden/io_steps.npz).  Everything is compared bitwise: the feature has no tolerance.  Shapes are the smallest that
reach every path: level side 4 (2x2 blocks, byte loads), 8 (exactly one 8-byte vector per row), 16 / 32 / 64 (several), the strided
gather of depth differences 1..3, one and three channels (planes at odd multiples of 16 and 64 bytes)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dataset_ref import make_stack, oracle_batch

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops
DS = pg.DeviceImageDataset
M = 7
# n, idx (0, M - 1 and a repeat among them), flip (mixed / all-zero / NULL / a mirrored single image)
DRAWS = [([3, 0, 6, 3, 1], [0, 1, 1, 0, 1]), ([0, 6, 0], [0, 0, 0]), ([6], None), ([6], [1]), ([2, 2, 5, 0, 6], None)]
RANGES = [((0, 255), (0, 255)), ((0, 255), (0, 25.5)), ((0, 255), (-1, 1)), ((0, 200), (-1, 1))]
ALPHAS = [1.0, 0.85, 0.3, 0.0]


def _fx():
    return np.load(os.path.join(GOLDEN, 'io_steps.npz'))


def _log2(v):
    return int(v).bit_length() - 1


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def device_batch(stack_d, idx, flip, dd, alpha, range_in=(0, 255), range_out=(-1, 1)):
    return ops.real_batch_u8(stack_d, dev(idx, torch.int64), None if flip is None else dev(flip, torch.uint8), dd, alpha, range_in, range_out,
                             check=True).cpu().numpy()


# --------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('S,dd', [(4, 0), (8, 0), (16, 0), (32, 0), (32, 1), (32, 2), (32, 3), (64, 1), (64, 2), (64, 3)])
def test_kernel_against_host_mode_and_oracle(S, dd, C):
    stack = make_stack(M, C, S)
    stack[M - 1, :, :2, :2] = 255                              # a level pixel of 255 at every depth difference: the (0, 200) clip acts
    stack_d = dev(stack)
    for idx, flip in DRAWS:
        for range_in, range_out in RANGES:
            for alpha in ALPHAS:
                want = oracle_batch(stack, idx, flip, dd, alpha, range_in, range_out)
                host = pg.dataset.batch_host(stack, idx, flip, dd, alpha, range_in, range_out)
                got = device_batch(stack_d, idx, flip, dd, alpha, range_in, range_out)
                case = (idx, flip, range_in, range_out, alpha)
                assert got.dtype == np.float32 and got.shape == (len(idx), C, S >> dd, S >> dd), case
                assert np.array_equal(host, want), case
                assert np.array_equal(got, want), case
    if dd:
        assert oracle_batch(stack, [M - 1], None, dd, 1.0, (0, 255), (0, 255)).max() == 255
        assert oracle_batch(stack, [M - 1], None, dd, 1.0, (0, 200), (0, 200)).max() == 200


def test_argument_checks():
    stack = dev(make_stack(2, 3, 8))
    idx = dev([0, 1], torch.int64)
    with pytest.raises(IndexError):
        ops.real_batch_u8(stack, dev([0, 2], torch.int64), check=True)
    with pytest.raises(IndexError):
        ops.real_batch_u8(stack, dev([-1, 0], torch.int64), check=True)
    for bad in (dict(stack_u8=stack.float()), dict(idx=idx.int()), dict(idx=idx.cpu()), dict(flip=dev([1], torch.uint8)),
                dict(stack_u8=stack[:, :, :, :4]), dict(idx=idx[:0])):
        with pytest.raises(ValueError):
            ops.real_batch_u8(**dict(dict(stack_u8=stack, idx=idx), **bad))
    lib, out = pg._lib.load(), torch.empty(2 * 3 * 8 * 8, device='cuda')
    call = lambda src, Mv, C, S, dd, ix, n, o: lib.pg_real_batch_u8(src, Mv, C, S, dd, ix, None, n, o, 1.0, 0.0, 255.0, -1.0, 1.0, None)
    s, i, o = stack.data_ptr(), idx.data_ptr(), out.data_ptr()
    assert call(None, 2, 3, 8, 0, i, 2, o) == call(s, 2, 3, 8, 0, None, 2, o) == call(s, 2, 3, 8, 0, i, 2, None) == -1
    assert call(s, 0, 3, 8, 0, i, 2, o) == call(s, 2, 3, 8, 0, i, 0, o) == call(s, 2, 2, 8, 0, i, 2, o) == call(s, 2, 3, 8, -1, i, 2, o) == -1
    assert call(s, 2, 3, 12, 0, i, 2, o) == call(s, 2, 3, 8, 3, i, 2, o) == -2            # S not a power of two; r = 1
    torch.cuda.synchronize()


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_golden_real_through_the_device_path(tag):
    fx = _fx()
    x, alpha = fx['real/%s/in' % tag], float(fx['real/%s/alpha' % tag])
    ds = DS(x, model_dataset_depth_offset=_log2(x.shape[-1]), shuffle=False, alpha=alpha)
    assert np.array_equal(ds.batch(len(x)).cpu().numpy(), fx['real/%s/out' % tag])
    assert np.array_equal(torch.stack([ds[i] for i in range(len(x))]).numpy(), fx['real/%s/out' % tag])


@pytest.mark.parametrize('tag', ['p2', 'p3'])
def test_golden_pyramid_through_the_device_path(tag):
    fx = _fx()
    x, diff = fx['pyr/%s/in' % tag], int(fx['pyr/%s/diff' % tag])
    ds = DS(x[None], model_dataset_depth_offset=_log2(x.shape[-1]) - diff, pyramid='direct', range_out=(0, 255), shuffle=False)
    assert np.array_equal(ds.batch(1).cpu().numpy()[0], fx['pyr/%s/out' % tag].astype(np.float32))


@pytest.mark.parametrize('S,dd', [(8, 0), (32, 0), (32, 1), (64, 2), (64, 3)])
@pytest.mark.parametrize('C', [1, 3])
def test_composition_identity(S, dd, C):
    """The new kernel == the two pinned ones around an index_select and a flip of the last axis."""
    stack_d = dev(make_stack(M, C, S, seed=1))
    for idx, flip in DRAWS:
        idx_d = dev(idx, torch.int64)
        for alpha, ranges in ((0.3, RANGES[2]), (1.0, RANGES[1]), (0.85, RANGES[3])):
            level = stack_d.index_select(0, idx_d)
            if dd:
                level = ops.pyramid_level_u8(level, dd, ranges[0])
            if flip is not None:
                level = torch.where(dev(flip, torch.bool).view(-1, 1, 1, 1), torch.flip(level, dims=[-1]), level).contiguous()
            want = ops.real_prepare_u8(level, alpha, *ranges)
            got = ops.real_batch_u8(stack_d, idx_d, None if flip is None else dev(flip, torch.uint8), dd, alpha, *ranges)
            assert torch.equal(got, want), (idx, flip, alpha, ranges)


# ------------------------------------------------------------------------------------------------- dataset object
def _pair(x, **kw):
    return DS(x, device='cuda', **kw), DS(x, device='cpu', **kw)


def test_chain_levels_on_the_device_are_host_modes():
    x = make_stack(5, 3, 64)
    d, h = _pair(x, pyramid='chain')
    assert sorted(d._levels) == sorted(h._levels) == [2, 3, 4, 5, 6]
    for depth in d._levels:
        assert d._levels[depth].is_cuda and torch.equal(d._levels[depth].cpu(), h._levels[depth])
    d.close()
    assert d._levels == {}


@pytest.mark.parametrize('pyramid', ['chain', 'direct'])
def test_device_and_host_twin_give_the_same_batches(pyramid):
    x = make_stack(M, 3, 32)
    d, h = _pair(x, pyramid=pyramid, mirror_augment=True, seed=4)
    f_d, f_h = d.metric_batches(), h.metric_batches()
    for k in range(12):                                        # 12 draws of 3 over M = 7: five epoch boundaries
        if k == 4:
            d.model_depth = h.model_depth = 2
            d.alpha = h.alpha = 0.25
        if k == 8:
            d.model_depth = h.model_depth = 3
            d.alpha = h.alpha = 0.0
        got = d.batch(3)
        assert got.is_cuda and torch.equal(got.cpu(), h.batch(3)), k
        if k % 5 == 0:
            assert torch.equal(f_d(4).cpu(), f_h(4)) and torch.equal(d[k % M], h[k % M])
    assert d.cursor == h.cursor == 36
    assert torch.equal(d.batch(2, alpha=0.5).cpu(), h.batch(2, alpha=0.5))


def test_batches_are_issued_on_the_current_stream_without_host_synchronisation(monkeypatch):
    x = make_stack(16, 3, 16)
    d, h = _pair(x, model_dataset_depth_offset=4, mirror_augment=True, seed=2, alpha=0.5)
    want = [h.batch(3) for _ in range(3)]
    first = d.batch(3)                                         # the epoch's upload happens here
    s = torch.cuda.Stream()
    streams, syncs = [], []
    monkeypatch.setattr(pg._lib, 'CALL_HOOK', lambda fn, args, name: (streams.append((name, args[-1])), fn(*args))[1])
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: syncs.append('synchronize'))
    for name in ('item', 'cpu', 'tolist', 'numpy'):
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _n=name, **k: syncs.append(_n))
    with torch.cuda.stream(s):
        got = [d.batch(3), d.batch(3)]
    monkeypatch.undo()
    assert syncs == []
    assert streams == [('pg_real_batch_u8', s.cuda_stream)] * 2 and s.cuda_stream != torch.cuda.default_stream().cuda_stream
    s.synchronize()                                            # ... and nothing else: the results are complete
    assert torch.equal(first.cpu(), want[0]) and torch.equal(got[0].cpu(), want[1]) and torch.equal(got[1].cpu(), want[2])


# ------------------------------------------------------------------------------------------------- in the trainer
def _train(ds, lookahead=False, run_kimg=None, monitor=False):
    torch.manual_seed(3)
    shape = (1, 3, 16, 16)
    kw = dict(fmap_base=64, fmap_max=16)
    G, D = pg.Generator(shape, latent_size=16, **kw).cuda(), pg.Discriminator(shape, **kw).cuda()
    opt_g = pg.FusedAdam(G.parameters(), 0.001, betas=(0.0, 0.99))
    opt_d = pg.FusedAdam(D.parameters(), 0.001, betas=(0.0, 0.99))
    seen = []

    def rlg(n):
        g = torch.Generator().manual_seed(5)
        return lambda: torch.randn(n, 16, generator=g)

    def d_loss(Dm, Gm, real, z):
        seen.append((real.clone(), int(real.shape[0]), ds.model_depth, ds.alpha))
        return pg.wgan_gp_D_loss(Dm, Gm, real, z)
    tr = pg.Trainer(D, G, d_loss, pg.wgan_gp_G_loss, opt_d, opt_g, ds, None, None, prefetch_inputs=lookahead)
    tr.register_plugin(pg.DepthManager(ds.loader, rlg, 2, minibatch_default=4, minibatch_overrides={1: 3, 2: 2}, lod_training_nimg=12,
                                       lod_transition_nimg=12))
    if monitor:
        g = torch.Generator().manual_seed(9)
        tr.register_plugin(pg.SWDMonitor(ds.metric_batches(), lambda n: torch.randn(n, 16, generator=g), num_images=32, minibatch=8,
                                         swd_ticks=1, patches_per_image=8, dir_repeats=1, dirs_per_repeat=16))
    if run_kimg is None:
        for _ in range(9):
            tr.train()
    else:
        tr.run(run_kimg)
    torch.cuda.synchronize()
    return seen, tr


@pytest.mark.parametrize('lookahead', [False, True])
def test_trainer_sees_the_batches_of_the_host_twin(lookahead):
    """The real batches that reach the D loss are the host twin's for the same (n, depth, alpha) sequence, faded ones included.
    ``prefetch_inputs=True`` looks ahead only for batches that have to be uploaded (trainer._InputPrefetch: "device-resident batches
    pass through untouched"), so no batch of a replaced loader is ever drawn and dropped: the sequence is the same one."""
    x = make_stack(11, 3, 16)
    kw = dict(mirror_augment=True, seed=6)
    seen, tr = _train(DS(x, **kw), lookahead)
    twin = DS(x, device='cpu', **kw)
    assert [(n, depth) for _, n, depth, _ in seen] == [(4, 0)] * 3 + [(3, 1)] * 6
    assert [alpha for _, _, _, alpha in seen] == [1.0] * 3 + [0.0, 0.25, 0.5, 0.75, 1.0, 1.0]
    for k, (real, n, depth, alpha) in enumerate(seen):
        twin.model_depth, twin.alpha = depth, alpha
        assert real.dtype == torch.float32 and torch.equal(real.cpu(), twin.batch(n)), k
    assert tr.dataset.cursor == twin.cursor == 30 and tr._inputs.hits == 0


def test_metric_does_not_move_the_training_stream():
    x = make_stack(11, 3, 16)
    plain, _ = _train(DS(x, seed=6), run_kimg=0.04)
    with_metric, tr = _train(DS(x, seed=6), run_kimg=0.04, monitor=True)
    assert tr.G.depth == 2 and tr.stats['swd']['val'] > 0 and 'swd_16' in tr.stats
    assert len(plain) == len(with_metric) == 13
    for (a, *sa), (b, *sb) in zip(plain, with_metric):
        assert sa == sb and torch.equal(a, b)
