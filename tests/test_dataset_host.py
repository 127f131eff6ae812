"""DeviceImageDataset in host mode (device='cpu'): the definition of the real-image batch against the reference's own outputs
(tests/golden/io_steps.npz) and the oracle, the index stream, the DepthDataset protocol.  Everything is compared bitwise."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dataset_ref import make_stack, oracle_batch, oracle_level

import pggan_amd as pg

DS = pg.DeviceImageDataset


def _fx():
    return np.load(os.path.join(GOLDEN, 'io_steps.npz'))


def _log2(v):
    return int(v).bit_length() - 1


def host(images, depth=None, **kw):
    """Host-mode dataset whose stage is dataset depth ``depth`` (default: the source level) at model_depth 0."""
    kw.setdefault('shuffle', False)
    off = _log2(images.shape[-1]) if depth is None else depth
    return DS(images, model_dataset_depth_offset=off, device='cpu', **kw)


# ------------------------------------------------------------------------------------------------ golden fixtures
@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
@pytest.mark.parametrize('pyramid', ['chain', 'direct'])
def test_source_level_batch_is_the_references_getitem(tag, pyramid):
    fx = _fx()
    x = fx['real/%s/in' % tag]
    ds = host(x, alpha=float(fx['real/%s/alpha' % tag]), pyramid=pyramid)
    out = ds.batch(len(x))
    assert out.dtype == torch.float32 and np.array_equal(out.numpy(), fx['real/%s/out' % tag])


@pytest.mark.parametrize('tag', ['p2', 'p3'])
def test_direct_level_is_the_references_datapoint(tag):
    fx = _fx()
    x, diff = fx['pyr/%s/in' % tag], int(fx['pyr/%s/diff' % tag])
    ds = host(x[None], depth=_log2(x.shape[-1]) - diff, pyramid='direct', range_out=(0, 255))
    assert np.array_equal(ds.batch(1).numpy()[0], fx['pyr/%s/out' % tag].astype(np.float32))


# --------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize('C,S', [(3, 32), (1, 64)])
def test_chain_and_direct_against_the_oracle(C, S):
    x = make_stack(5, C, S)
    top = _log2(S)
    chain = {top: x}
    for d in range(top - 1, 0, -1):
        chain[d] = oracle_level(chain[d + 1], 1)
    differ = []
    for depth in range(top, 1, -1):
        for alpha in (0.0, 0.3, 1.0):
            got = host(x, depth, pyramid='chain', alpha=alpha).batch(5).numpy()
            assert np.array_equal(got, oracle_batch(chain[depth], range(5), None, 0, alpha)), (depth, alpha)
            got_d = host(x, depth, pyramid='direct', alpha=alpha).batch(5).numpy()
            assert np.array_equal(got_d, oracle_batch(x, range(5), None, top - depth, alpha)), (depth, alpha)
            if top - depth <= 1:
                assert np.array_equal(got, got_d)
            elif alpha == 1.0:
                differ.append(not np.array_equal(got, got_d))
    assert differ and all(differ)                              # box-mean chain vs 4-sample subsampling: two levels down they part


def test_levels_kept_by_chain_mode():
    x = make_stack(3, 3, 32)
    ds = host(x, depth=2, pyramid='chain')
    assert sorted(ds._levels) == [2, 3, 4, 5]
    level = x
    for d in (4, 3, 2):
        level = oracle_level(level, 1)
        assert np.array_equal(ds._levels[d].numpy(), level)
    assert sorted(host(x, depth=2, pyramid='direct')._levels) == [5]


@pytest.mark.parametrize('depthdiff', [0, 1, 2])
def test_mirror_acts_on_the_level_image(depthdiff):
    x = make_stack(4, 3, 16)
    idx, flip = np.array([3, 0, 3, 1]), np.array([1, 0, 0, 1], dtype=np.uint8)
    for alpha in (0.3, 1.0):
        got = pg.dataset.batch_host(x, idx, flip, depthdiff, alpha)
        assert np.array_equal(got, oracle_batch(x, idx, flip, depthdiff, alpha))
        plain = pg.dataset.batch_host(x, idx, None, depthdiff, alpha)
        assert np.array_equal(got[0], plain[0][..., ::-1]) and np.array_equal(got[1], plain[1])   # fade and mirror commute
    if depthdiff > 1:                                          # ... and mirroring the SOURCE first is something else
        other = pg.dataset.batch_host(x[..., ::-1], idx, None, depthdiff, 1.0)
        assert not np.array_equal(other[0], pg.dataset.batch_host(x, idx, flip, depthdiff, 1.0)[0])


def test_range_in_clips_the_level_bytes():
    x = make_stack(2, 1, 16)
    got = pg.dataset.batch_host(x, [0, 1], None, 1, 1.0, (0, 200), (0, 200))
    assert got.max() == 200.0 and np.array_equal(got, oracle_batch(x, [0, 1], None, 1, 1.0, (0, 200), (0, 200)))
    got = pg.dataset.batch_host(x, [0, 1], None, 2, 0.3, (0, 200), (-1, 1))
    assert np.array_equal(got, oracle_batch(x, [0, 1], None, 2, 0.3, (0, 200), (-1, 1)))


# --------------------------------------------------------------------------------------------------- index stream
def _stream(ds, sizes):
    out = [ds.draw_indices(n) for n in sizes]
    idx = torch.cat([i for i, _ in out])
    return idx, (torch.cat([f for _, f in out]) if out[0][1] is not None else None)


def test_every_epoch_is_a_permutation_and_the_seed_decides():
    x = make_stack(7, 1, 4)
    a, _ = _stream(host(x, shuffle=True, seed=3), [7, 7, 7])
    for e in range(3):
        assert sorted(a[7 * e:7 * e + 7].tolist()) == list(range(7))
    assert not torch.equal(a[:7], a[7:14])
    b, _ = _stream(host(x, shuffle=True, seed=3), [21])
    c, _ = _stream(host(x, shuffle=True, seed=4), [21])
    assert torch.equal(a, b) and not torch.equal(a, c)
    g = torch.Generator().manual_seed(3)                       # the reference's InfiniteRandomSampler, train.py:51-56
    assert torch.equal(a, torch.cat([torch.randperm(7, generator=g) for _ in range(3)]))
    s, f = _stream(host(x, shuffle=False), [10])
    assert s.tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1, 2] and f is None


def test_stream_does_not_depend_on_batch_sizes_or_loaders():
    x = make_stack(7, 1, 4)
    one = host(x, shuffle=True, seed=1, mirror_augment=True)
    idx, flip = one.draw_indices(9)
    ds = host(x, shuffle=True, seed=1, mirror_augment=True)
    twin = host(x, shuffle=True, seed=1, mirror_augment=True)
    l1 = ds.loader(4)
    got = [next(l1)]
    l2 = ds.loader(3)                                          # what DepthManager does at a stage change
    got += [next(l2), ds.batch(2)]
    assert ds.cursor == 9 == one.cursor
    want = torch.from_numpy(pg.dataset.batch_host(x, idx.numpy(), flip.numpy(), 0, 1.0))
    assert torch.equal(torch.cat(got), want)
    i2, f2 = _stream(twin, [4, 3, 2])
    assert torch.equal(i2, idx) and torch.equal(f2, flip)


def test_batch_across_an_epoch_boundary_and_flags_at_positions():
    x = make_stack(7, 1, 4)
    g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(6)
    perms = torch.cat([torch.randperm(7, generator=g) for _ in range(3)])
    flags = torch.cat([torch.randint(0, 2, (7,), generator=g2, dtype=torch.uint8) for _ in range(3)])
    ds = host(x, shuffle=True, seed=5, mirror_augment=True)
    for k in range(4):                                         # the 2nd draw is positions 5..9: tail of epoch 0, head of epoch 1
        idx, flip = ds.draw_indices(5)
        assert torch.equal(idx, perms[5 * k:5 * k + 5]) and torch.equal(flip, flags[5 * k:5 * k + 5]) and flip.dtype == torch.uint8
    assert ds.cursor == 20
    assert host(x, shuffle=True, seed=5).draw_indices(5)[1] is None          # no flags drawn without mirror_augment


def test_ranks_draw_disjoint_parts_of_the_same_positions():
    x = make_stack(8, 1, 4)
    ref, _ = _stream(host(x, shuffle=True, seed=2), [16])
    r0, r1 = (host(x, shuffle=True, seed=2, rank=k, world=2) for k in (0, 1))
    seen = []
    for step in range(4):                                      # 2n = 4 divides M = 8: two steps are one epoch
        a, b = r0.draw_indices(2)[0], r1.draw_indices(2)[0]
        assert torch.equal(torch.cat([a, b]), ref[4 * step:4 * step + 4])
        seen += a.tolist() + b.tolist()
        assert r0.cursor == r1.cursor == 4 * (step + 1)
    assert sorted(seen[:8]) == list(range(8)) and sorted(seen[8:]) == list(range(8))
    with pytest.raises(ValueError):
        host(x, rank=2, world=2)


def test_metric_batches_leave_the_training_cursor_alone():
    x = make_stack(7, 3, 16)
    ds = host(x, depth=3, shuffle=True, seed=0, mirror_augment=True, alpha=0.4)
    twin = host(x, depth=3, shuffle=True, seed=0, mirror_augment=True, alpha=0.4)
    f = ds.metric_batches()
    first = ds.batch(3)
    m = f(5)
    assert ds.cursor == 3 and f.stream.cursor == 5 and tuple(m.shape) == (5, 3, 8, 8)
    g = torch.Generator().manual_seed(1)
    assert np.array_equal(m.numpy(), oracle_batch(ds._levels[3].numpy(), torch.randperm(7, generator=g)[:5].numpy(), None, 0, 1.0))
    assert torch.equal(first, twin.batch(3)) and torch.equal(ds.batch(6), twin.batch(6))


# ------------------------------------------------------------------------------------------ protocol and signature
def test_protocol():
    x = make_stack(5, 3, 16)
    ds = host(x, depth=2, alpha=0.3, pyramid='direct')
    assert ds.shape == (5, 3, 16, 16) and len(ds) == 5
    assert ds.model_depth == 0 and ds.alpha == 0.3
    ds.model_depth = 1
    item = ds[4]
    assert item.dtype == torch.float32 and tuple(item.shape) == (3, 8, 8)
    assert np.array_equal(item.numpy(), oracle_batch(x, [4], None, 1, 0.3)[0])
    ds.alpha = 1.0
    assert np.array_equal(ds[-1].numpy(), oracle_batch(x, [4], None, 1, 1.0)[0])
    with pytest.raises(IndexError):
        ds[5]
    assert len(list(ds)) == 5                                  # the sequence protocol ends: a plain DataLoader works
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2)))
    assert np.array_equal(batch.numpy(), oracle_batch(x, [0, 1], None, 1, 1.0))
    ds.model_depth = 3
    with pytest.raises(ValueError):
        ds.batch(1)
    assert DS(x, max_images=3, device='cpu').shape == (3, 3, 16, 16)
    assert DS(torch.from_numpy(x), device='cpu').shape == (5, 3, 16, 16)
    ds.close()
    with pytest.raises(RuntimeError):
        ds.batch(1)
    assert 'DeviceImageDataset' in pg.__all__ and pg.dataset.DeviceImageDataset is DS


def test_value_errors():
    good = make_stack(2, 3, 8)
    for bad in (make_stack(2, 3, 8)[:, :2], np.zeros((2, 3, 12, 12), np.uint8), good.astype(np.float32), torch.zeros(2, 3, 8, 8),
                np.zeros((2, 3, 8, 16), np.uint8), np.zeros((2, 3, 2, 2), np.uint8), good[0], [[1]]):
        with pytest.raises(ValueError):
            DS(bad, device='cpu')
    for kw in (dict(max_images=0), dict(max_images=1.5), dict(max_images=-2), dict(pyramid='box'), dict(world=0)):
        with pytest.raises(ValueError):
            DS(good, device='cpu', **kw)


def test_from_npy(tmp_path):
    x = make_stack(3, 3, 8)
    np.save(str(tmp_path / 'stack.npy'), x)
    ds = DS.from_npy(str(tmp_path / 'stack.npy'), model_dataset_depth_offset=3, shuffle=False, device='cpu')
    assert np.array_equal(ds.batch(3).numpy(), oracle_batch(x, range(3), None, 0, 1.0))


def test_from_folder(tmp_path):
    import PIL.Image as PIL                                    # (utils.DeviceImageSaver needs it too)
    x = make_stack(3, 3, 8)
    folder = tmp_path / 'images'
    folder.mkdir()
    for i in (2, 0, 1):
        PIL.fromarray(x[i].transpose(1, 2, 0), 'RGB').save(str(folder / ('im%d.png' % i)))
    rgb = DS.from_folder(str(folder), imread_mode='RGB', model_dataset_depth_offset=3, shuffle=False, device='cpu')
    assert rgb.shape == (3, 3, 8, 8) and np.array_equal(rgb._levels[3].numpy(), x)
    assert DS.from_folder(str(folder), device='cpu').shape == (3, 1, 8, 8)         # 'L', the reference's default


def test_signature():
    P, I, L, D = pg._lib.P, pg._lib.I, pg._lib.L, pg._lib.D
    assert pg._lib.SIGNATURES['pg_real_batch_u8'] == [P, L, I, I, I, P, P, I, P, D, D, D, D, D, P]
    assert pg._lib.ABI_VERSION == 27                           # additive: the version stays
    assert callable(pg.ops.real_batch_u8)
