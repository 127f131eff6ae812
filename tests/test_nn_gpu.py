"""The nearest-neighbour search on the MI355X (csrc/nn_search.hip through ops.quantize_u8 / l2dist_u8 / topk_smallest_i64 / nn_search_u8,
metrics.NearestNeighbours, plugins.NNMonitor) against its numpy int64 statement tests/nn_ref.py.  Integer arithmetic: EVERY comparison
is ``==``, there is no tolerance anywhere.

Shapes are the smallest at which each part can go wrong.  The distance kernel works on 128 bytes of every image per step, 32 images per
wave, 128 per workgroup and 32 queries per MFMA tile, at most ops.NN_MAX_QUERIES per launch: image sizes 16 and 48 are less than a step,
192 is one and a half, 3072 a whole number; the image counts run from one to several workgroups, ragged against the wave and the
workgroup; the query counts from one to one more than a launch takes.  3x256x256 is past the 2^17 terms an int32 accumulator holds and
3x512x512 is split over 192 slices of D.  The stack and the queries always differ, and the forced bytes 0, 127, 128, 255 sit either
side of the shift by 128."""
import os
import types

import numpy as np
import pytest
import torch

import msssim_ref
import nn_ref
from dataset_ref import make_stack
from redzone import Redzone

pytestmark = pytest.mark.gpu

SIZES = [(1, 4), (3, 4), (3, 8), (3, 32)]                    # D = 16, 48, 192, 3072
COUNTS = [1, 31, 33, 65, 100, 129, 300]                      # the issue's five, and two that take more than one 128-image workgroup


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def query_counts(pg):
    return [1, 5, 33, pg.ops.NN_MAX_QUERIES + 1]


_queries = {}


def queries_for(pg, C, r):
    """NN_MAX_QUERIES + 1 query images of a size, made once; a test takes the first K."""
    if (C, r) not in _queries:
        _queries[(C, r)] = nn_ref.images(pg.ops.NN_MAX_QUERIES + 1, C, r, seed=500 + 10 * r + C)
    return _queries[(C, r)]


# ------------------------------------------------------------------------------------------------------------ pg_l2dist_u8
@pytest.mark.parametrize('C,r', SIZES)
@pytest.mark.parametrize('M', COUNTS)
def test_l2dist_tails_and_ragged_tiles(pg, C, r, M):
    stack = nn_ref.images(M, C, r, seed=100 + M)
    queries = queries_for(pg, C, r)
    want = nn_ref.l2dist(stack, queries)
    stack_d = dev(stack)
    for K in query_counts(pg):
        got = pg.ops.l2dist_u8(stack_d, dev(queries[:K]))
        assert got.dtype == torch.int64 and tuple(got.shape) == (K, M)
        assert np.array_equal(got.cpu().numpy(), want[:K]), (C, r, M, K)
    # a planted copy is at distance exactly 0, a row/column swap cannot pass: stack != queries and K != M
    stack[M // 2] = queries[3]
    got = pg.ops.l2dist_u8(dev(stack), dev(queries[:5])).cpu().numpy()
    assert got[3, M // 2] == 0 and np.array_equal(got, nn_ref.l2dist(stack, queries[:5]))


def test_l2dist_writes_into_out(pg):
    stack, queries = nn_ref.images(40, 3, 4, seed=1), nn_ref.images(70, 3, 4, seed=2)
    out = torch.full((70, 40), -7, dtype=torch.int64, device='cuda')
    assert pg.ops.l2dist_u8(dev(stack), dev(queries), out=out) is out
    assert np.array_equal(out.cpu().numpy(), nn_ref.l2dist(stack, queries))


def test_l2dist_beyond_the_int32_accumulator(pg):
    """D = 196608 > 2^17: the cross term alone reaches 3.2e9 > 2^31 and a distance 1.28e10 > 2^32."""
    C, r = 3, 256
    D = C * r * r
    stack = np.stack([np.zeros((C, r, r), np.uint8), np.full((C, r, r), 255, np.uint8), nn_ref.images(1, C, r, seed=9)[0]])
    queries = np.stack([np.zeros((C, r, r), np.uint8), np.full((C, r, r), 255, np.uint8)])
    got = pg.ops.l2dist_u8(dev(stack), dev(queries)).cpu().numpy()
    want = nn_ref.l2dist(stack, queries)
    assert want[0, 1] == want[1, 0] == 255 * 255 * D > 2 ** 32 and want[0, 0] == want[1, 1] == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize('M,C,r,K', [(2, 3, 512, 3), (4096, 1, 4, 5)])
def test_l2dist_split_over_d_and_over_many_workgroups(pg, M, C, r, K):
    stack, queries = nn_ref.images(M, C, r, seed=21), nn_ref.images(K, C, r, seed=22)
    stack_d, queries_d = dev(stack), dev(queries)
    got = pg.ops.l2dist_u8(stack_d, queries_d)
    assert np.array_equal(got.cpu().numpy(), nn_ref.l2dist(stack, queries))
    assert torch.equal(pg.ops.l2dist_u8(stack_d, queries_d), got)            # integer atomics: the same bits again


# ---------------------------------------------------------------------------------------------------- pg_topk_smallest_i64
@pytest.mark.parametrize('M', [1, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_topk_ties_go_to_the_lower_index(pg, M):
    """Rows of few distinct values (every value is planted many times), one row of distinct values past 2^32, one constant row, one
    descending row (the k smallest are the LAST elements a thread sees) -- for k = 1, k = 16 (or M below 16) and two in between."""
    rs = np.random.RandomState(M)
    rows = [rs.randint(0, 4, size=M), rs.randint(0, max(2, M // 8), size=M), rs.permutation(M).astype(np.int64) * 3 + (1 << 33),
            np.full(M, 12345678901), np.arange(M)[::-1].copy(), rs.randint(0, 2, size=M).astype(np.int64) << 40]
    dist = np.stack(rows).astype(np.int64)
    dist_d = dev(dist)
    for k in sorted({1, min(M, 3), min(M, 7), min(M, 16)}):                # (the kernel keeps lists of 1, 4, 8 or 16)
        values, indices = pg.ops.topk_smallest_i64(dist_d, k)
        want_v, want_i = nn_ref.topk_smallest(dist, k)
        assert values.dtype == indices.dtype == torch.int64 and tuple(values.shape) == tuple(indices.shape) == (len(rows), k)
        assert np.array_equal(values.cpu().numpy(), want_v) and np.array_equal(indices.cpu().numpy(), want_i), (M, k)
    assert np.array_equal(pg.ops.topk_smallest_i64(dist_d, 1)[1].cpu().numpy()[3], [0])          # a constant row: index 0


# ---------------------------------------------------------------------------------------------------------- pg_quantize_u8
@pytest.mark.parametrize('drange', [(-1, 1), (0, 1), (-2.5, 3.0)])
@pytest.mark.parametrize('shape', [(2, 3, 4, 4), (1, 1, 5, 7), (3, 3, 16, 16)])
def test_quantize_is_the_saved_image_bit_for_bit(pg, drange, shape):
    lo, hi = drange
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(n)
    x = lo + (hi - lo) * (torch.rand(n, generator=g, dtype=torch.float32) * 1.2 - 0.1)           # a tenth of the range outside at both ends
    halves = lo + (torch.arange(0, min(n, 256), dtype=torch.float64) + 0.5) * ((hi - lo) / 255.0)   # as close to the .5 ties as fp32 gets
    x[:halves.numel()] = halves.float()
    x[-1], x[-2] = hi + 100.0, lo - 100.0
    x = x.view(shape)
    want = msssim_ref.quantise(x, drange).numpy()
    assert want.min() == 0 and want.max() == 255
    got = pg.ops.quantize_u8(x.cuda(), drange)
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8))
    # ... and exactly the bytes of the grid the saver writes
    grid = pg.ops.image_grid_u8(x.cuda()[:1], drange)                                            # one image: [h, w, C]
    assert np.array_equal(grid.cpu().numpy().transpose(2, 0, 1), got.cpu().numpy()[0])


def test_quantize_exact_halves(pg):
    x = torch.tensor([0.5, 1.5, 2.5, 127.5, 254.5, 255.5, -0.5, 3.0], dtype=torch.float32)      # drange (0, 255): the scale is 1
    got = pg.ops.quantize_u8(x.view(1, 1, 2, 4).cuda(), (0, 255)).cpu().view(-1).tolist()
    assert got == [0, 2, 2, 128, 254, 255, 0, 3]
    assert got == msssim_ref.quantise(x, (0, 255)).to(torch.uint8).tolist()


# -------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('pyramid', ['chain', 'direct'])
def test_nearest_neighbours_over_a_device_dataset(pg, pyramid):
    M, k = 70, 4
    stack = make_stack(M, 3, 32, seed=4)
    ds = pg.DeviceImageDataset(stack, pyramid=pyramid, model_initial_depth=1)                    # 8x8: two levels below the source
    twin = pg.DeviceImageDataset(stack, pyramid=pyramid, model_initial_depth=1, device='cpu')
    level = ds.level_stack()
    assert level.is_cuda and tuple(level.shape) == (M, 3, 8, 8)
    assert np.array_equal(level.cpu().numpy(), twin.level_stack().numpy())
    js = [5, 69, 0, 33]
    idx = torch.tensor(js, device='cuda')
    samples = pg.ops.real_batch_u8(level, idx)                                                   # training images as G would emit them
    flipped = pg.ops.real_batch_u8(level, idx, torch.ones(4, dtype=torch.uint8, device='cuda'))
    fresh = torch.rand(3, 3, 8, 8, generator=torch.Generator().manual_seed(3)).cuda() * 2 - 1
    batch = torch.cat([samples, flipped, fresh])
    for mirror in (False, True):
        nn = pg.metrics.NearestNeighbours(ds, k=k, mirror=mirror)
        res = nn.search(batch)
        assert res['index'][:4, 0].tolist() == js and res['sqdist'][:4, 0].tolist() == [0] * 4 and not res['mirrored'][:4, 0].any()
        if mirror:
            assert res['index'][4:8, 0].tolist() == js and res['sqdist'][4:8, 0].tolist() == [0] * 4 and res['mirrored'][4:8, 0].all()
        else:
            assert (res['sqdist'][4:8, 0] > 0).all() and not res['mirrored'].any()
        again = nn.search(batch)
        host = pg.metrics.NearestNeighbours(twin, k=k, mirror=mirror).search(batch.cpu())
        q = msssim_ref.quantise(batch.cpu()).numpy().astype(np.uint8)
        want = nn_ref.search_mirror(level.cpu().numpy(), q, k) if mirror else nn_ref.search(level.cpu().numpy(), q, k) + (np.zeros((11, k), bool),)
        for name, ref in zip(('sqdist', 'index', 'mirrored'), want):
            assert torch.equal(res[name], again[name]) and torch.equal(res[name], host[name])
            assert np.array_equal(res[name].numpy(), ref)
        assert torch.equal(res['rms'], host['rms']) and res['rms'].dtype == torch.float64
        near = nn.neighbours(res)
        assert near.is_cuda and tuple(near.shape) == (11, k, 3, 8, 8)
        assert torch.equal(near[:4, 0], samples) and torch.equal(near.cpu(), pg.metrics.NearestNeighbours(twin, k=k, mirror=mirror).neighbours(host))
        if mirror:
            assert torch.equal(near[4:8, 0], flipped)
    ds.model_depth = 3                                                                           # the search follows the stage
    res = pg.metrics.NearestNeighbours(ds, k=1).search(pg.ops.real_batch_u8(ds.level_stack(), idx))
    assert res['index'][:, 0].tolist() == js and res['sqdist'][:, 0].tolist() == [0] * 4


def test_monitor_epoch_on_a_tiny_network(pg, tmp_path, deterministic_forward):
    torch.manual_seed(11)
    G = pg.Generator((1, 3, 16, 16), latent_size=32, fmap_base=128, fmap_max=32).to('cuda')
    G.depth = 2
    stack = make_stack(40, 3, 16, seed=7)
    ds = pg.DeviceImageDataset(stack, model_initial_depth=2, mirror_augment=True)
    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=7000, G=G, g_ema=None)
    g = torch.Generator().manual_seed(5)
    drawn = []

    def sample_fn(n):
        drawn.append(torch.randn(n, 32, generator=g))
        return drawn[-1]

    saver = pg.utils.DeviceImageSaver(str(tmp_path), resolution=None)
    mon = pg.NNMonitor(ds, sample_fn, num_samples=9, k=3, nn_ticks=1, postprocessors=(saver,))
    mon.register(trainer)
    mon.epoch(1)
    st = trainer.stats
    assert set(st) == {'nn_rms', 'nn_rms_min'} and [z.shape[0] for z in drawn] == [9]
    samples = G.forward(drawn[0].cuda())
    res = pg.metrics.NearestNeighbours(ds, k=3, mirror=True).search(samples)
    rms = res['rms'][:, 0].numpy()
    assert st['nn_rms']['val'] == float(rms.mean()) and st['nn_rms_min']['val'] == float(rms.min()) and 0 < rms.min() <= 255
    import PIL.Image
    png = os.path.join(str(tmp_path), 'fakes_nn_000007.png')
    sheet = np.asarray(PIL.Image.open(png))
    assert sheet.shape == (4 * 16, 4 * 16, 3)
    # row i of the sheet: sample i, then its three neighbours as the search named them
    q = pg.ops.quantize_u8(samples).cpu().numpy()
    for i in range(4):
        assert np.array_equal(sheet[16 * i:16 * i + 16, :16].transpose(2, 0, 1), q[i])
        for j in range(3):
            image = stack[int(res['index'][i, j])]
            if bool(res['mirrored'][i, j]):
                image = image[..., ::-1]
            assert np.array_equal(sheet[16 * i:16 * i + 16, 16 * (j + 1):16 * (j + 2)].transpose(2, 0, 1), image)


# ------------------------------------------------------------------------------------------------------------- guard bands
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


@pytest.mark.parametrize('M,K,C,r', [(33, 5, 3, 4), (130, 65, 3, 8), (3, 2, 3, 64)])
def test_l2dist_inside_guard_bands(pg, rz, M, K, C, r):
    """Ragged in images and queries with a tail in D; two launches and two workgroups; split over D (atomics into the zeroed output)."""
    stack, queries = nn_ref.images(M, C, r, seed=31), nn_ref.images(K, C, r, seed=32)
    stack_d, queries_d = rz.guard(torch.from_numpy(stack), name='stack'), rz.guard(torch.from_numpy(queries), name='queries')
    assert stack_d.data_ptr() % 32 == 16
    got = pg.ops.l2dist_u8(stack_d, queries_d)
    chk(rz)                                                    # bands intact, inputs unchanged, every output element written
    assert np.array_equal(got.cpu().numpy(), nn_ref.l2dist(stack, queries))


def test_topk_inside_guard_bands(pg, rz):
    dist = np.random.RandomState(4).randint(0, 50, size=(3, 261)).astype(np.int64)
    dist_d = rz.guard(torch.from_numpy(dist), name='dist')
    values, indices = pg.ops.topk_smallest_i64(dist_d, 16)
    chk(rz)
    want = nn_ref.topk_smallest(dist, 16)
    assert np.array_equal(values.cpu().numpy(), want[0]) and np.array_equal(indices.cpu().numpy(), want[1])


@pytest.mark.parametrize('shape', [(1, 3, 5, 7), (2, 3, 4, 4)])
def test_quantize_inside_guard_bands(pg, rz, shape):
    """(an odd element count: the byte kernel; a multiple of four: the packed one.)  The output's sentinel byte 0xA5 = 165 is a legal
    level, so the inputs avoid it."""
    levels = np.random.RandomState(6).randint(0, 256, size=shape)
    levels[levels == 0xA5] = 0xA4
    x = torch.from_numpy((levels / 127.5 - 1).astype(np.float32))
    want = msssim_ref.quantise(x).numpy().astype(np.uint8)
    assert np.array_equal(want, levels) and not (want == 0xA5).any()
    got = pg.ops.quantize_u8(rz.guard(x, name='images'))
    chk(rz)
    assert np.array_equal(got.cpu().numpy(), want)
