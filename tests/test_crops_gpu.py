"""pg_crop_batch_u8 (csrc/real_batch.hip: the batch kernels with strips as their source) and ``DeviceStripDataset`` on the device.  The
kernel is defined by an equality: its batch is, bit for bit, ``ops.real_batch_u8`` of the same windows materialised as a stack -- so
every comparison here is ``==``, against that and against ``dataset.batch_host``.  The dataset is held against its ``device='cpu'``
twin batch for batch, and against ``DeviceImageDataset`` on square strips."""
import numpy as np
import pytest
import torch

from crops_ref import all_starts, check_items, check_square_strips_equal_the_stack, make_strips, windows
from dataset_ref import make_stack

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops, ds_mod = pg.ops, pg.dataset
StripLevel, DeviceStripDataset = pg.dataset.StripLevel, pg.dataset.DeviceStripDataset


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# shift in {0, 1, 2} with depthdiff 0, depthdiff in {0, 1, 2} with shift 0
@pytest.mark.parametrize('shift,dd', [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2)])
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('R', [4, 8, 16, 32])
def test_kernel_equals_real_batch_of_the_materialised_windows(R, C, shift, dd):
    if R >> dd < 2:
        with pytest.raises(RuntimeError, match='PG_E_ALIGN'):
            ops.crop_batch_u8(StripLevel.pack(make_strips(C, R), 'cuda'), dev(np.zeros(1, np.int64)), dev(np.zeros(1, np.int64)),
                              depthdiff=dd)
        return
    strips = make_strips(C, R, seed=R + C)                                            # R, 2R, 3R columns: pitches 16, 32, 48, 64, 96
    level = StripLevel.pack(strips, 'cuda')
    table = level.table.cpu().numpy()
    assert np.all(table[:, :2] % 16 == 0) and np.all(table[:, 1] >= table[:, 2]) and table[:, 2].tolist() == [R, 2 * R, 3 * R]
    if R == 8:
        assert table[:, 1].tolist() == [16, 16, 32]                                   # padded rows
    idx, u = all_starts(strips, R)
    n = idx.size
    assert idx[-1] == 2 and u[-1] == 2 * R and (R < 16 or set((u % 16).tolist()) == set(range(16)))
    rng = np.random.RandomState(R + 10 * C + shift)
    pos = (u << shift) | rng.randint(0, 1 << shift, size=n)                           # the low bits are shifted out
    mixed = rng.randint(0, 2, size=n).astype(np.uint8)
    stack = windows(strips, idx, u, R)
    stack_d, arange_d, idx_d, pos_d = dev(stack), torch.arange(n, device='cuda'), dev(idx), dev(pos)
    for flip in (mixed, None):
        flip_d = None if flip is None else dev(flip)
        for alpha in (0.3, 1.0):
            for range_out in ((-1, 1), (0, 255)):
                got = ops.crop_batch_u8(level, idx_d, pos_d, flip_d, shift, dd, alpha, (0, 255), range_out, check=True)
                assert got.dtype == torch.float32 and tuple(got.shape) == (n, C, R >> dd, R >> dd)
                want = ops.real_batch_u8(stack_d, arange_d, flip_d, dd, alpha, (0, 255), range_out)
                assert torch.equal(got, want)
                assert np.array_equal(got.cpu().numpy(), ds_mod.batch_host(stack, np.arange(n), flip, dd, alpha, (0, 255), range_out))


def test_range_in_clips_the_level_bytes_as_real_batch_does():
    strips = make_strips(3, 16, seed=9)
    level = StripLevel.pack(strips, 'cuda')
    idx, u = all_starts(strips, 16)
    stack = windows(strips, idx, u, 16)
    got = ops.crop_batch_u8(level, dev(idx), dev(u), None, 0, 1, 0.5, (10, 200), (-1, 1))
    assert torch.equal(got, ops.real_batch_u8(dev(stack), torch.arange(idx.size, device='cuda'), None, 1, 0.5, (10, 200), (-1, 1)))
    assert np.array_equal(got.cpu().numpy(), ds_mod.batch_host(stack, np.arange(idx.size), None, 1, 0.5, (10, 200), (-1, 1)))


@pytest.mark.parametrize('pyr', ['chain', 'direct'])
@pytest.mark.parametrize('C,R', [(1, 8), (2, 16), (3, 32)])
def test_dataset_equals_its_host_twin(C, R, pyr):
    strips = make_strips(C, R, extra=5, seed=3)
    kw = dict(pyramid=pyr, mirror_augment=True, seed=4, alpha=0.4, model_initial_depth=1)
    a, b = DeviceStripDataset(strips, device='cuda', **kw), DeviceStripDataset(strips, device='cpu', **kw)
    assert a.shape == b.shape == (6, C, R, R) and a.lengths == b.lengths
    assert torch.equal(a.level_stack().cpu(), b.level_stack())
    for n in (4, 5, 3):                                                               # 12 positions: two epochs of 6
        x, y = a.batch(n), b.batch(n)
        assert x.is_cuda and tuple(x.shape) == (n, C, 8, 8) and np.array_equal(x.cpu().numpy(), y.numpy())
    for depth, alpha in ((0, 0.7), (_top(R), 1.0)):                                   # a stage change: DepthManager writes both, makes a loader
        a.model_depth = b.model_depth = depth
        a.alpha = b.alpha = alpha
        la, lb = a.loader(5), b.loader(5)
        for _ in range(2):
            assert np.array_equal(next(la).cpu().numpy(), next(lb).numpy())
        assert torch.equal(a.level_stack().cpu(), b.level_stack())
        assert np.array_equal(a[3].numpy(), b[3].numpy())
    assert a.cursor == b.cursor == 32
    fa, fb = a.metric_batches(seed=2), b.metric_batches(seed=2)
    assert np.array_equal(fa(7).cpu().numpy(), fb(7).numpy()) and a.cursor == 32
    if pyr == 'chain':
        assert a.level_bytes()[_top(R) + 2] >= b.level_bytes()[_top(R) + 2] and sorted(a.level_bytes()) == sorted(b.level_bytes())
    a.close()
    with pytest.raises(RuntimeError):
        a.batch(1)


# r = 4 and every 'direct' stage below R take the blocks kernel, r >= 8 at depth difference 0 the rows kernel: both kernels of both sources
@pytest.mark.parametrize('pyr', ['chain', 'direct'])
@pytest.mark.parametrize('C,R', [(1, 8), (2, 16), (3, 32)])
def test_square_strips_are_the_image_dataset(C, R, pyr):
    check_square_strips_equal_the_stack(pg, C, R, pyr, 'cuda')


@pytest.mark.parametrize('pyr', ['chain', 'direct'])
def test_items_are_the_getitem_tensors(pyr):
    check_items(DeviceStripDataset(make_strips(2, 16, seed=8), pyramid=pyr, seed=2, device='cuda'), (0, 2))
    images = pg.DeviceImageDataset(make_stack(5, 3, 16, seed=9), pyramid=pyr, seed=2, device='cuda')
    idx = check_items(images, (0, 2))
    for depth in (0, 2):                                                              # what _make(idx, None, 1.0) gave: the stage's stack
        images.model_depth = depth
        stack, _, dd = images._stage()
        assert torch.equal(images.items(idx), ops.real_batch_u8(stack, idx, None, dd, 1.0, images.range_in, images.range_out))


def _top(R):
    return R.bit_length() - 1 - 2                                                     # model_depth of the source resolution (offset 2)


def test_nearest_neighbours_find_a_window_of_the_set():
    ds = DeviceStripDataset(make_strips(2, 16, seed=6), model_initial_depth=1, device='cuda')
    nn = pg.NearestNeighbours(source=ds)
    assert tuple(nn.stack().shape) == (6, 2, 8, 8)
    res = nn.search(torch.stack([ds[4], ds[1]]).cuda())
    assert res['index'].reshape(-1).tolist() == [4, 1] and res['sqdist'].reshape(-1).tolist() == [0, 0]


def _waveform(nsamp, seed):
    return (np.random.RandomState(seed).rand(nsamp).astype(np.float32) - 0.5)


def test_spectrogram_strip_reproduces_the_analysis():
    n_fft, hop = 32, 8
    y = _waveform(hop * (3 * n_fft // 2), 1)                                          # 49 frames: a strip of 48 columns
    logmag, ifreq = pg.phase.analyse(dev(y), n_fft, hop, n_fft // 2, None)
    image = pg.phase.magif_u8(logmag, ifreq, pg.phase.default_mag_range(n_fft))[0]
    assert tuple(image.shape) == (2, 16, 49)
    strip = pg.spectrogram_strip_u8(y, n_fft, hop)
    assert strip.is_cuda and strip.dtype == torch.uint8 and strip.is_contiguous() and tuple(strip.shape) == (2, 16, 48)
    assert torch.equal(strip, image[:, :, 1:])
    mono = pg.spectrogram_strip_u8(y, n_fft, hop, img_mode='abslog')
    assert tuple(mono.shape) == (1, 16, 48) and torch.equal(mono[:, :, :16], image[:1, :, 1:17])
    # two channels are mixed down as spectrogram_u8 does it: sum / 2
    stereo = np.stack([y, y], axis=1)
    assert torch.equal(pg.spectrogram_strip_u8(stereo, n_fft, hop), strip)
    with pytest.raises(ValueError):
        pg.spectrogram_strip_u8(y, n_fft, hop, img_mode='reallog')


def test_from_waveforms_with_two_lengths():
    n_fft, hop = 32, 8
    ys = [_waveform(hop * 48, 2), _waveform(hop * 16 + 5, 3)]
    ds = DeviceStripDataset.from_waveforms(ys, n_fft, hop, 'magif', None, seed=1, mirror_augment=True)
    assert ds.shape == (4, 2, 16, 16) and ds.lengths == [48, 16]
    strips = [pg.spectrogram_strip_u8(y, n_fft, hop).cpu().numpy() for y in ys]
    twin = DeviceStripDataset(strips, seed=1, mirror_augment=True, device='cpu')
    for n in (3, 3):
        assert np.array_equal(ds.batch(n).cpu().numpy(), twin.batch(n).numpy())
    mono = DeviceStripDataset.from_waveforms(ys, n_fft, hop, 'abslog', (0.0, 3.0), shuffle=False)
    assert mono.shape == (4, 1, 16, 16)
    with pytest.raises(ValueError, match='waveform 1'):
        DeviceStripDataset.from_waveforms([ys[0], _waveform(hop * 16 - 1, 4)], n_fft, hop)


def test_errors():
    strips = make_strips(1, 8)
    level = StripLevel.pack(strips, 'cuda')
    zero = dev(np.zeros(2, np.int64))
    big = torch.zeros(level.buffer.numel() + 16, dtype=torch.uint8, device='cuda')
    off = StripLevel(big[1:1 + level.buffer.numel()], level.table, 1, 8, level.cols)
    assert off.buffer.data_ptr() % 16 == 1
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):                             # misaligned base
        ops.crop_batch_u8(off, zero, zero)
    with pytest.raises(RuntimeError, match='PG_E_ARG'):                               # C = 4
        ops.crop_batch_u8(StripLevel(level.buffer, level.table, 4, 8, level.cols), zero, zero)
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):                             # r < 2
        ops.crop_batch_u8(level, zero, zero, depthdiff=3)
    with pytest.raises(IndexError, match='idx'):
        ops.crop_batch_u8(level, dev(np.array([0, 3])), zero, check=True)
    with pytest.raises(IndexError, match='idx'):
        ops.crop_batch_u8(level, dev(np.array([-1, 0])), zero, check=True)
    with pytest.raises(IndexError, match='pos'):                                      # strip 1 has 16 columns: start 9 leaves it
        ops.crop_batch_u8(level, dev(np.array([1, 1])), dev(np.array([8, 9])), check=True)
    with pytest.raises(IndexError, match='pos'):                                      # ... and so does 18 >> 1
        ops.crop_batch_u8(level, dev(np.array([1, 1])), dev(np.array([17, 18])), shift=1, check=True)
    with pytest.raises(IndexError, match='pos'):
        ops.crop_batch_u8(level, dev(np.array([0, 2])), dev(np.array([0, -1])), check=True)
    assert tuple(ops.crop_batch_u8(level, dev(np.array([1, 2])), dev(np.array([8, 16])), check=True).shape) == (2, 1, 8, 8)
    with pytest.raises(ValueError):
        ops.crop_batch_u8(level, zero, dev(np.zeros(3, np.int64)))
    with pytest.raises(ValueError):
        ops.crop_batch_u8(level, zero.to(torch.int32), zero)
