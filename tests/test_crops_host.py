"""The crop stream and the host twin of ``DeviceStripDataset`` (no GPU): the draws, the windows and the protocol are held against
``dataset.level_host`` / ``prepare_host`` / ``batch_host`` on windows sliced here.  Every comparison is ``==``."""
import numpy as np
import pytest
import torch

from crops_ref import check_items, check_square_strips_equal_the_stack, make_strips, pyramid, windows
from dataset_ref import make_stack

import pggan_amd as pg

ds_mod = pg.dataset
CropStream, DeviceStripDataset = pg.dataset.CropStream, pg.dataset.DeviceStripDataset
R = 8
LENGTHS = (R, 2 * R, 3 * R)


def drain(stream, sizes, **kw):
    parts = [stream.take(n, **kw) for n in sizes]
    return tuple(None if parts[0][k] is None else torch.cat([p[k] for p in parts]).numpy() for k in range(3))


# ----------------------------------------------------------------------------------------------------------- CropStream
def test_same_seed_same_draws_and_the_seed_decides():
    a = drain(CropStream(LENGTHS, R, seed=3, flags=True), [13])
    b = drain(CropStream(LENGTHS, R, seed=3, flags=True), [13])
    c = drain(CropStream(LENGTHS, R, seed=4, flags=True), [13])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))
    assert a[0].dtype == np.int64 and a[1].dtype == np.int64 and a[2].dtype == np.uint8
    assert drain(CropStream(LENGTHS, R, seed=3), [2])[2] is None


def test_unshuffled_epoch_enumerates_the_windows():
    s = CropStream(LENGTHS, R, shuffle=False)
    assert s.P == 6
    idx, pos, _ = drain(s, [6, 6])
    assert idx.tolist() == [0, 1, 1, 2, 2, 2] * 2
    assert pos.tolist() == [0, 0, R, 0, R, 2 * R] * 2


def test_draws_do_not_depend_on_batch_sizes():
    a = drain(CropStream(LENGTHS, R, seed=1, flags=True), [20])
    b = drain(CropStream(LENGTHS, R, seed=1, flags=True), [1, 4, 2, 7, 6])           # crosses epoch boundaries (P = 6) inside a draw
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_ranks_take_disjoint_positions():
    whole = drain(CropStream(LENGTHS, R, seed=5, flags=True), [16])
    ranks = [CropStream(LENGTHS, R, seed=5, flags=True) for _ in range(2)]
    got = [[], []]
    for _ in range(2):
        for rk, s in enumerate(ranks):
            got[rk].append(s.take(4, rank=rk, world=2))
    assert ranks[0].cursor == ranks[1].cursor == 16
    for k in range(3):
        order = [got[0][0][k], got[1][0][k], got[0][1][k], got[1][1][k]]             # positions 0-3, 4-7, 8-11, 12-15
        assert np.array_equal(torch.cat(order).numpy(), whole[k])


def test_strip_choice_formula_on_a_hand_computed_case():
    """Strips of R, 2R, 3R columns, R = 8: w = (1, 9, 17), W = 27, cumsum = (1, 10, 27).  p = floor(g 27): p = 0 -> strip 0,
    1 <= p <= 9 -> strip 1, 10 <= p <= 26 -> strip 2; start = floor(f w)."""
    s = CropStream(LENGTHS, R, seed=11)
    idx, pos, _ = drain(s, [s.P])
    g = torch.rand(s.P, dtype=torch.float64, generator=torch.Generator().manual_seed(11)).numpy()
    f = torch.rand(s.P, dtype=torch.float64, generator=torch.Generator().manual_seed(12)).numpy()
    for j in range(s.P):
        p = min(int(np.floor(g[j] * 27)), 26)
        strip = 0 if p == 0 else 1 if p <= 9 else 2
        w = (1, 9, 17)[strip]
        assert idx[j] == strip and pos[j] == min(int(np.floor(f[j] * w)), w - 1)
    # the ends of the formula, by the arithmetic alone
    cum = np.cumsum([1, 9, 17])
    assert [int(np.searchsorted(cum, p, side='right')) for p in (0, 1, 9, 10, 26)] == [0, 1, 1, 2, 2]
    assert min(int(np.floor(np.nextafter(1.0, 0.0) * 27)), 26) == 26


def test_starts_stay_inside_every_level():
    lengths = (16, 48, 32)
    s = CropStream(lengths, 16, seed=2)
    idx, pos, _ = drain(s, [10 * s.P])
    assert pos.min() >= 0 and set(idx.tolist()) == {0, 1, 2}
    for k in range(4):                                                                # r = 16 .. 2
        cols_k, r = np.asarray(lengths)[idx] >> k, 16 >> k
        assert np.all((pos >> k) <= cols_k - r)
    # the last legal start of a strip survives every shift
    for T in lengths:
        for k in range(4):
            assert (T - 16) >> k == (T >> k) - (16 >> k)


def test_stream_value_errors():
    with pytest.raises(ValueError):
        CropStream((), R)
    with pytest.raises(ValueError):
        CropStream((R, R - 1), R)
    with pytest.raises(ValueError):
        CropStream(LENGTHS, R).take(0)


# ------------------------------------------------------------------------------------------- DeviceStripDataset, host mode
def host(strips, **kw):
    kw.setdefault('device', 'cpu')
    return DeviceStripDataset(strips, **kw)


def tiles(strips, S):
    return np.concatenate([windows([s], [0] * (s.shape[2] // S), [i * S for i in range(s.shape[2] // S)], S) for s in strips])


def test_truncation_shape_and_len():
    strips = make_strips(2, R, extra=3)                                               # R + 3, 2R + 3, 3R + 3 columns
    ds = host(strips)
    assert ds.lengths == [R, 2 * R, 3 * R]
    assert ds.shape == (6, 2, R, R) and len(ds) == 6
    cut = [s[:, :, :t] for s, t in zip(strips, ds.lengths)]
    ds.model_depth = 1
    assert np.array_equal(ds.level_stack().numpy(), tiles(cut, R))
    assert ds.level_bytes() == {2: 2 * 4 * 24, 3: 2 * 8 * 48}
    # torch tensors are taken as well
    assert np.array_equal(host([torch.from_numpy(s) for s in strips], model_initial_depth=1).level_stack().numpy(), tiles(cut, R))


def test_value_errors():
    good = make_strips(1, R)
    for bad, word in (([], 'at least one'), ([good[0].astype(np.float32)], 'strip 0'), ([good[0][0]], 'strip 0'),
                      ([good[0], good[1][:, :, :R - 1]], 'strip 1'), ([good[0], make_strips(2, R)[1]], 'strip 1'),
                      ([good[0], make_strips(1, 2 * R)[0]], 'strip 1'), ([np.zeros((4, R, R), np.uint8)], 'channels'),
                      ([np.zeros((1, 6, 12), np.uint8)], 'rows'), ([np.zeros((1, 2, 12), np.uint8)], 'rows')):
        with pytest.raises(ValueError, match=word):
            host(bad)
    with pytest.raises(ValueError, match='pyramid'):
        host(good, pyramid='box')
    with pytest.raises(ValueError, match='rank'):
        host(good, rank=2, world=2)
    ds = host(good, model_initial_depth=5)
    with pytest.raises(ValueError, match='dataset depth'):
        ds.batch(1)
    with pytest.raises(IndexError):
        host(good)[6]


@pytest.mark.parametrize('pyr', ['chain', 'direct'])
@pytest.mark.parametrize('C', [1, 2, 3])
def test_getitem_is_the_references_tensor_of_window_i(C, pyr):
    strips = make_strips(C, R, seed=1)
    ds = host(strips, pyramid=pyr, alpha=0.3, range_out=(-1, 1))
    full = tiles(strips, R)
    for depth, dd in ((1, 0), (0, 1)):
        ds.model_depth = depth
        for i in range(len(ds)):
            want = ds_mod.prepare_host(ds_mod.level_host(full[i], dd), 0.3, (0, 255), (-1, 1))
            got = ds[i]
            assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
        assert np.array_equal(ds[-1].numpy(), ds[len(ds) - 1].numpy())


def test_chain_is_repeated_level_host_of_the_strip():
    strips = make_strips(3, 16, seed=2)
    ds = host(strips, pyramid='chain', model_dataset_depth_offset=1, shuffle=False)
    for depth in range(4):                                                            # sides 2, 4, 8, 16
        k = 3 - depth
        ds.model_depth = depth
        below = pyramid(strips, k, ds_mod.level_host)
        assert np.array_equal(ds.level_stack().numpy(), tiles(below, 16 >> k))
        # ... and a crop at start t reads columns t >> k of that level
        idx, pos = np.array([2, 1, 2]), np.array([32, 5, 13])
        got = ds._make(torch.from_numpy(idx), torch.from_numpy(pos), None, 1.0).numpy()
        want = ds_mod.batch_host(windows(below, idx, pos >> k, 16 >> k), np.arange(3), None, 0, 1.0)
        assert np.array_equal(got, want)


def test_chain_and_direct_agree_at_the_source_and_one_level_below():
    strips = make_strips(2, 16, seed=3)
    a, b = (host(strips, pyramid=p, shuffle=False, mirror_augment=True, alpha=0.6) for p in ('chain', 'direct'))
    for depth, same in ((2, True), (1, True), (0, False)):
        a.model_depth = b.model_depth = depth
        assert np.array_equal(a.level_stack().numpy(), b.level_stack().numpy()) == same
        assert np.array_equal(a.batch(6).numpy(), b.batch(6).numpy()) == same
        assert np.array_equal(a[4].numpy(), b[4].numpy()) == same


@pytest.mark.parametrize('pyr', ['chain', 'direct'])
def test_batches_are_batch_host_of_the_windows(pyr):
    strips = make_strips(3, R, seed=4)
    ds = host(strips, pyramid=pyr, seed=7, mirror_augment=True, alpha=0.3, model_initial_depth=0)
    ref = CropStream(ds.lengths, R, seed=7, flags=True)
    for n in (4, 5):                                                                  # the second draw crosses the epoch boundary
        idx, pos, flip = (t.numpy() for t in ref.take(n))
        if pyr == 'chain':
            want = ds_mod.batch_host(windows(pyramid(strips, 1, ds_mod.level_host), idx, pos >> 1, R // 2), np.arange(n), flip, 0, 0.3)
        else:
            want = ds_mod.batch_host(windows(strips, idx, pos, R), np.arange(n), flip, 1, 0.3)
        got = ds.batch(n)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3, R // 2, R // 2)
        assert np.array_equal(got.numpy(), want)
    assert ds.cursor == 9


def test_stage_change_continues_the_stream():
    strips = make_strips(1, R, seed=5)
    ds, twin = host(strips, seed=9), CropStream((R, 2 * R, 3 * R), R, seed=9)
    l1 = ds.loader(3)
    b1 = next(l1)
    ds.model_depth, ds.alpha = 1, 0.5                                                 # what DepthManager writes at a stage change ...
    l2 = ds.loader(2)                                                                 # ... and the loader it makes then
    b2 = next(l2)
    assert tuple(b1.shape) == (3, 1, 4, 4) and tuple(b2.shape) == (2, 1, 8, 8) and ds.cursor == 5
    twin.take(3)
    idx, pos, _ = (None if t is None else t.numpy() for t in twin.take(2))
    assert np.array_equal(b2.numpy(), ds_mod.batch_host(windows(strips, idx, pos, R), np.arange(2), None, 0, 0.5))


def test_metric_batches_leave_the_training_cursor_alone():
    ds = host(make_strips(1, R, seed=6), alpha=0.2, mirror_augment=True)
    f = ds.metric_batches(seed=3)
    got = f(4)
    assert ds.cursor == 0 and f.stream.cursor == 4
    idx, pos, flip = CropStream(ds.lengths, R, seed=3).take(4)
    assert flip is None
    want = ds_mod.batch_host(windows(pyramid(make_strips(1, R, seed=6), 1, ds_mod.level_host), idx.numpy(), pos.numpy() >> 1, R // 2),
                             np.arange(4), None, 0, 1.0)
    assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize('pyr', ['chain', 'direct'])
@pytest.mark.parametrize('C,side', [(1, 8), (2, 16), (3, 32)])
def test_square_strips_are_the_image_dataset(C, side, pyr):
    check_square_strips_equal_the_stack(pg, C, side, pyr, 'cpu')


@pytest.mark.parametrize('pyr', ['chain', 'direct'])
def test_items_are_the_getitem_tensors(pyr):
    strips = host(make_strips(2, 16, seed=8), pyramid=pyr, seed=2)
    check_items(strips, (0, 2))
    images = pg.DeviceImageDataset(make_stack(5, 3, 16, seed=9), pyramid=pyr, seed=2, device='cpu')
    idx = check_items(images, (0, 2))
    for depth in (0, 2):                                                              # what _make(idx, None, 1.0) gave: the stage's stack
        images.model_depth = depth
        stack, _, dd = images._stage()
        assert np.array_equal(images.items(idx).numpy(), ds_mod.batch_host(stack.numpy(), idx.numpy(), None, dd, 1.0))


def test_projection_monitor_takes_a_strip_dataset():
    ds = host(make_strips(2, 16, seed=10), model_initial_depth=1)
    m = pg.ProjectionMonitor(source=ds, num_images=4)
    t = m.targets(8)
    assert t.dtype == torch.float32 and tuple(t.shape) == (4, 2, 8, 8)
    assert torch.equal(t, torch.stack([ds[i] for i in (2, 3, 4, 5)])) and ds.cursor == 0
    with pytest.raises(ValueError, match='7 targets'):
        pg.ProjectionMonitor(source=ds, num_images=7)


def test_close():
    ds = host(make_strips(1, R))
    ds.close()
    with pytest.raises(RuntimeError):
        ds.batch(1)
    with pytest.raises(RuntimeError):
        ds.level_stack()


def test_strip_level_layout():
    rows, total = ds_mod.StripLevel.layout(3, 4, [4, 8, 12, 20])
    assert rows == [(0, 16, 4), (192, 16, 8), (384, 16, 12), (576, 32, 20)] and total == 576 + 3 * 4 * 32
    assert all(o % 16 == 0 and p % 16 == 0 and p >= c for o, p, c in rows)


# ------------------------------------------------------------------------------------------------------------ the binding
def test_binding_parses_the_crop_header_and_leaves_the_product_header_alone():
    lib = pg._lib
    assert len(lib.SIGNATURES) == 96 and len(lib.CONSTANTS) == 27 and lib.ABI_VERSION == 27
    assert list(lib.CROP_SIGNATURES) == ['pg_crop_batch_u8']
    P, I, L, D = lib.P, lib.I, lib.L, lib.D
    assert lib.CROP_SIGNATURES['pg_crop_batch_u8'] == [P, P, L, I, I, I, I, P, P, P, I, P, D, D, D, D, D, P]
    assert lib.CROP_CONSTANTS == {'PG_CROP_TABLE_WORDS': 3, 'PG_CROP_PITCH_ALIGN': 16}
    assert not set(lib.CROP_SIGNATURES) & set(lib.SIGNATURES)


def test_exports():
    assert pg.DeviceStripDataset is DeviceStripDataset and pg.CropStream is CropStream
    assert pg.spectrogram_strip_u8 is pg.sound.spectrogram_strip_u8
    assert {'DeviceStripDataset', 'CropStream', 'spectrogram_strip_u8'} <= set(pg.__all__)
    assert pg.sound.strip_frames(1000, 128) == 7
