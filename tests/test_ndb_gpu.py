"""The k-means kernels on the MI355X (csrc/cluster.hip through cluster.assign_u8 / cluster_sums_u8 / centroids_u8, metrics.NDB,
plugins.NDBMonitor) against tests/ndb_ref.py and against the numpy twin.  Integer arithmetic: EVERY comparison is ``==``.

Shapes are the smallest at which each part can go wrong.  The sums kernel gives a workgroup a slice of min(D / 16, 64) pieces of 16 bytes
and 256 / that many rows of member images: D = 16 is 256 rows of one piece, 48 is 85 rows of three with a thread left over, 3072 and
4096 are 4 rows of 64 pieces in 3 and 4 slices, 12288 is 12 slices.  Image counts run from one to more than a workgroup's rows; a member
list is shared between workgroups (the zeroing launch and the atomics) only above 2048 members per bin at D = 16, which the 5000- and
20000-image cases reach."""
import types

import numpy as np
import pytest
import torch

import ndb_ref
from dataset_ref import make_stack

pytestmark = pytest.mark.gpu

SIZES = [(1, 4), (3, 4), (3, 32), (1, 64), (3, 64)]          # D = 16, 48, 3072, 4096, 12288
COUNTS = [1, 37, 130, 257]
BINS = [2, 3, 50, 64]


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def images(n, C, r, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, C, r, r)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ assign_u8
@pytest.mark.parametrize('C,r', SIZES)
def test_assign_against_the_reference(pg, C, r):
    stack = images(COUNTS[-1], C, r, seed=10 * r + C)
    cents = images(BINS[-1], C, r, seed=10 * r + C + 1)
    cents[1] = cents[0]                                          # two equal centroids: bin 1 stays empty
    cents[5] = stack[3]                                          # a centroid that IS an image: distance 0
    for M in COUNTS:
        for K in BINS:
            label, best = pg.cluster.assign_u8(dev(stack[:M]), dev(cents[:K]))
            want_l, want_d = ndb_ref.assign(stack[:M], cents[:K])
            assert label.dtype == torch.int32 and best.dtype == torch.int64 and tuple(label.shape) == tuple(best.shape) == (M,)
            assert label.cpu().tolist() == want_l and best.cpu().tolist() == want_d, (C, r, M, K)
            assert 1 not in want_l
    assert want_l[3] == 5 and want_d[3] == 0


def test_assign_an_all_equal_stack_and_all_equal_centroids(pg):
    stack = np.full((130, 3, 4, 4), 7, dtype=np.uint8)
    cents = np.full((50, 3, 4, 4), 9, dtype=np.uint8)
    label, best = pg.cluster.assign_u8(dev(stack), dev(cents))
    assert label.cpu().tolist() == [0] * 130 and best.cpu().tolist() == [4 * 48] * 130       # every distance ties: bin 0
    cents[17] = 7
    label, best = pg.cluster.assign_u8(dev(stack), dev(cents))
    assert label.cpu().tolist() == [17] * 130 and best.cpu().tolist() == [0] * 130


# ------------------------------------------------------------------------------------------------------ cluster_sums_u8
def check_sums(pg, stack, labels, K):
    labels = np.asarray(labels, dtype=np.int32)
    sums, counts = pg.cluster.cluster_sums_u8(dev(stack), dev(labels), K)
    want_s, want_n = ndb_ref.sums(stack, labels.tolist(), K)
    assert sums.dtype == torch.int32 and counts.dtype == torch.int64 and tuple(sums.shape) == (K,) + stack.shape[1:]
    assert counts.cpu().tolist() == want_n
    assert np.array_equal(sums.cpu().numpy().astype(np.int64), want_s)
    return sums, counts


@pytest.mark.parametrize('C,r', SIZES)
def test_sums_against_the_reference(pg, C, r):
    stack = images(COUNTS[-1], C, r, seed=20 * r + C)
    rs = np.random.RandomState(r + C)
    for M in COUNTS:
        K = 5
        check_sums(pg, stack[:M], rs.randint(0, K, size=M), K)                               # random
        check_sums(pg, stack[:M], np.full(M, 3), K)                                          # all in one bin, the others empty
        check_sums(pg, stack[:M], np.array([-1, 0, 2])[rs.randint(0, 3, size=M)], K)         # non-members and empty bins
        check_sums(pg, stack[:M], rs.randint(-1, 64, size=M), 64)
    check_sums(pg, stack[:37], np.full(37, -1), 2)                                           # no member at all: zeros


def test_sums_member_lists_shared_between_workgroups(pg):
    stack = images(5000, 1, 4, seed=1)
    a, _ = check_sums(pg, stack, np.zeros(5000), 1)                                          # one bin of 5000 at D = 16: two shares
    b, _ = check_sums(pg, stack, np.zeros(5000), 1)
    assert torch.equal(a, b)                                                                 # integer atomics: the same bits again
    stack = images(20000, 1, 4, seed=2)
    labels = np.random.RandomState(3).randint(-1, 3, size=20000)
    labels[labels == 1] = 0                                                                  # bins of ~10000 and ~5000, bin 1 empty
    check_sums(pg, stack, labels, 3)


def test_sums_three_members_split_over_slices(pg):
    stack = images(9, 3, 64, seed=4)
    check_sums(pg, stack, [-1, 1, -1, -1, 1, -1, 0, 1, -1], 2)


def test_sums_argument_errors(pg):
    stack = dev(images(4, 1, 4, seed=5))
    with pytest.raises(ValueError):
        pg.cluster.cluster_sums_u8(stack, torch.zeros(4, dtype=torch.int64, device='cuda'), 2)          # int32 labels
    with pytest.raises(ValueError):
        pg.cluster.cluster_sums_u8(stack, torch.full((4,), 2, dtype=torch.int32, device='cuda'), 2)     # a label >= K
    with pytest.raises(ValueError):
        pg.cluster.cluster_sums_u8(stack, torch.full((4,), -2, dtype=torch.int32, device='cuda'), 2)
    with pytest.raises(ValueError):
        pg.cluster.cluster_sums_u8(dev(images(4, 1, 2, seed=5)), torch.zeros(4, dtype=torch.int32, device='cuda'), 2)   # D = 4
    label = torch.zeros(4, dtype=torch.int32, device='cuda')
    off = torch.tensor([0, 4, 4], dtype=torch.int32, device='cuda')
    out = torch.zeros((2, 16), dtype=torch.int32, device='cuda')
    s = pg.ops._stream()
    for args, err in (((stack.data_ptr(), 4, 16, label.data_ptr(), 5, off.data_ptr(), 2, out.data_ptr(), s), 'PG_E_ARG'),      # n > M
                      ((stack.data_ptr(), 4, 16, label.data_ptr(), 4, off.data_ptr(), 65, out.data_ptr(), s), 'PG_E_ARG'),
                      ((stack.data_ptr(), 4, 16, None, 4, off.data_ptr(), 2, out.data_ptr(), s), 'PG_E_ARG'),
                      ((stack.data_ptr(), 4, 24, label.data_ptr(), 4, off.data_ptr(), 2, out.data_ptr(), s), 'PG_E_ALIGN'),
                      ((stack.data_ptr() + 8, 3, 16, label.data_ptr(), 3, off.data_ptr(), 2, out.data_ptr(), s), 'PG_E_ALIGN')):
        with pytest.raises(RuntimeError, match=err):
            pg._lib.call('pg_cluster_sums_u8', *args)
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                                         # refused before any launch


def test_accumulator_bound(pg):
    """2^23 images of 16 bytes of 255 in one bin: every sum is 255 * 2^23 = 2 139 095 040 < 2^31, the centroid 255; one image more is
    refused."""
    M = pg.cluster.MAX_IMAGES
    assert M == 2 ** 23
    stack = torch.full((M, 1, 4, 4), 255, dtype=torch.uint8, device='cuda')
    label = torch.zeros(M, dtype=torch.int32, device='cuda')
    sums, counts = pg.cluster.cluster_sums_u8(stack, label, 2)
    assert counts.cpu().tolist() == [M, 0]
    assert sums.cpu().view(2, 16).tolist() == [[2139095040] * 16, [0] * 16]
    previous = torch.full((2, 1, 4, 4), 3, dtype=torch.uint8, device='cuda')
    new = pg.cluster.centroids_u8(sums, counts, previous)
    assert new.cpu().view(2, 16).tolist() == [[255] * 16, [3] * 16] and previous.cpu().view(-1).tolist() == [3] * 32
    del stack, label
    stack = torch.zeros((M + 1, 1, 4, 4), dtype=torch.uint8, device='cuda')
    label = torch.zeros(M + 1, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        pg.cluster.cluster_sums_u8(stack, label, 2)
    off = torch.tensor([0, M + 1, M + 1], dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg._lib.call('pg_cluster_sums_u8', stack.data_ptr(), M + 1, 16, label.data_ptr(), M + 1, off.data_ptr(), 2, sums.data_ptr(),
                     pg.ops._stream())


def test_sums_address_images_past_four_gib(pg):
    """70 000 images of 1x256x256 are 4.59e9 bytes > 2^32: the members sit past the 4 GiB boundary (image 65536 starts at 2^32), the
    rest of the stack is zero and mostly not a member, so the expected sums are those few images'."""
    M, C, r = 70000, 1, 256
    stack = torch.zeros((M, C, r, r), dtype=torch.uint8, device='cuda')
    assert stack.numel() > 2 ** 32
    where = [65535, 65536, 65537, 69999, 12]
    planted = images(len(where), C, r, seed=6)
    for j, m in enumerate(where):
        stack[m].copy_(dev(planted[j]))
    label = torch.full((M,), -1, dtype=torch.int32)
    label[[65535, 65537, 12, 100, 66000]] = 0                    # 100 and 66000 are zero images
    label[[65536, 69999]] = 1
    sums, counts = pg.cluster.cluster_sums_u8(stack, label.cuda(), 2)
    p = planted.astype(np.int64)
    assert counts.cpu().tolist() == [5, 2]
    assert np.array_equal(sums.cpu().numpy().astype(np.int64), np.stack([p[0] + p[2] + p[4], p[1] + p[3]]))


# --------------------------------------------------------------------------------------------------------- centroids_u8
def test_centroids_round_half_up(pg):
    K, D = 6, 16
    counts = [2, 3, 0, 2 ** 23, 1, 7]
    sums = np.zeros((K, 1, 4, 4), dtype=np.int64)
    sums[0].reshape(-1)[:] = [1, 3, 0, 2, 509, 510, 255, 5, 7, 9, 11, 13, 15, 17, 19, 21]      # halves exactly: .5 goes UP
    sums[1].reshape(-1)[:] = [4, 5, 0, 1, 2, 3, 764, 765, 763, 6, 7, 8, 9, 10, 11, 12]          # thirds either side of .5
    sums[2].reshape(-1)[:] = 77                                                              # count 0: ignored, the centroid is kept
    sums[3].reshape(-1)[:] = [255 * 2 ** 23, 2 ** 22, 2 ** 22 - 1, 0] * 4                    # 2 sums = 2^32 - 2^24; .5 exactly and just below
    sums[4].reshape(-1)[:] = np.arange(240, 256)
    sums[5].reshape(-1)[:] = [3, 4, 24, 25, 1781, 1782, 1785, 0, 10, 11, 17, 18, 31, 32, 38, 39]
    previous = images(K, 1, 4, seed=7)
    want = ndb_ref.centroids(sums, counts, previous)
    assert want[0].reshape(-1).tolist()[:6] == [1, 2, 0, 1, 255, 255] and want[3].reshape(-1).tolist()[:4] == [255, 1, 0, 0]
    assert np.array_equal(want[2], previous[2])
    got = pg.cluster.centroids_u8(dev(sums.astype(np.int32)), dev(np.array(counts, dtype=np.int64)), dev(previous))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------- metrics.NDB
def same_fit(a, b):
    assert torch.equal(a.labels.cpu(), b.labels.cpu()) and a.labels.dtype == b.labels.dtype == torch.int32
    assert torch.equal(a.centroids.cpu(), b.centroids.cpu()) and a.centroids.dtype == torch.uint8
    assert a.ref.tolist() == b.ref.tolist() and (a.iterations, a.converged, a.resolution) == (b.iterations, b.converged, b.resolution)


def same_result(a, b):
    assert a['gen'].tolist() == b['gen'].tolist() and a['ref'].tolist() == b['ref'].tolist() and a['ndb'] == b['ndb']
    assert a['jsd'].hex() == b['jsd'].hex() and np.array_equal(a['z'], b['z']) and a['ndb_over_k'] == b['ndb_over_k']


@pytest.mark.parametrize('blobs,per_blob,C,r,K,h', [(6, 40, 1, 16, 6, 0), (10, 24, 3, 8, 16, 48)])
def test_ndb_on_the_device_equals_the_twin_and_the_reference(pg, blobs, per_blob, C, r, K, h):
    centres = ndb_ref.planted_centres(blobs, C, r, 3)
    x = ndb_ref.planted_images(centres, per_blob, 4)
    want = ndb_ref.fit(x, K, h, 0)
    twin = pg.metrics.NDB(torch.from_numpy(x), k=K, holdout=h, device='cpu').fit()
    ndb = pg.metrics.NDB(dev(x), k=K, holdout=h).fit()
    assert ndb.centroids.is_cuda and ndb.labels.is_cuda
    same_fit(ndb, twin)
    assert ndb.labels.cpu().tolist() == want['labels'] and np.array_equal(ndb.centroids.cpu().numpy(), want['centroids'])
    assert ndb.ref.tolist() == want['ref'] and (ndb.iterations, ndb.converged) == (want['iterations'], want['converged'])
    first = (ndb.labels.clone(), ndb.centroids.clone(), ndb.ref.copy(), ndb.iterations)
    ndb.fit()                                                                                # the fit again: bit for bit
    assert torch.equal(ndb.labels, first[0]) and torch.equal(ndb.centroids, first[1]) and ndb.ref.tolist() == first[2].tolist()
    assert ndb.iterations == first[3]
    fresh = ndb_ref.planted_images(centres, 20, 77, drop=(1,))
    twin.feed_u8(torch.from_numpy(fresh))
    host = twin.result()
    assert host['gen'].tolist() == ndb_ref.histogram(fresh, want['centroids'])
    for batch in (1, 16, 64):
        ndb.reset()
        for a in range(0, fresh.shape[0], batch):
            ndb.feed_u8(dev(fresh[a:a + batch]))
        same_result(ndb.result(), host)
    as_fp32 = torch.from_numpy(fresh.astype(np.float32) / 127.5 - 1)
    ndb.reset()
    ndb.feed(as_fp32.cuda())
    same_result(ndb.result(), host)
    with pytest.raises(ValueError):
        ndb.reset() or ndb.feed(torch.zeros((2, C, 2 * r, 2 * r), device='cuda'))


def test_ndb_max_iter_one_on_the_device(pg):
    x = ndb_ref.planted_images(ndb_ref.planted_centres(6, 1, 16, 3), 40, 4)
    same_fit(pg.metrics.NDB(dev(x), k=6, max_iter=1).fit(), pg.metrics.NDB(torch.from_numpy(x), k=6, max_iter=1, device='cpu').fit())


@pytest.mark.parametrize('pyramid', ['chain', 'direct'])
def test_ndb_over_a_device_dataset(pg, pyramid):
    stack = make_stack(90, 3, 32, seed=4)
    ds = pg.DeviceImageDataset(stack, pyramid=pyramid, model_initial_depth=1)                # 8x8: two levels below the source
    twin_ds = pg.DeviceImageDataset(stack, pyramid=pyramid, model_initial_depth=1, device='cpu')
    ndb = pg.metrics.NDB(ds, k=7, holdout=20, seed=3).fit()
    twin = pg.metrics.NDB(twin_ds, k=7, holdout=20, seed=3, device='cpu').fit()
    assert ndb.resolution == 8 and tuple(ndb.centroids.shape) == (7, 3, 8, 8)
    same_fit(ndb, twin)
    samples = torch.rand(33, 3, 8, 8, generator=torch.Generator().manual_seed(3)) * 2 - 1
    ndb.feed(samples.cuda())
    twin.feed(samples)
    same_result(ndb.result(), twin.result())
    ds.model_depth = twin_ds.model_depth = 2                                                 # the fit follows the stage
    same_fit(ndb.fit(), twin.fit())
    assert ndb.resolution == 16


def test_monitor_on_a_tiny_network_through_a_stage_change(pg, deterministic_forward):
    torch.manual_seed(11)
    G = pg.Generator((1, 3, 16, 16), latent_size=32, fmap_base=128, fmap_max=32).to('cuda')
    G.depth = 1
    ds = pg.DeviceImageDataset(make_stack(60, 3, 16, seed=7), model_initial_depth=1)
    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=7000, G=G, g_ema=None)
    g = torch.Generator().manual_seed(5)
    drawn = []

    def sample_fn(n):
        drawn.append(torch.randn(n, 32, generator=g))
        return drawn[-1]

    mon = pg.NDBMonitor(ds, sample_fn, num_samples=40, minibatch=16, k=5, ndb_ticks=1)
    mon.register(trainer)
    for depth, resolution in ((1, 8), (1, 8), (2, 16)):
        G.depth = ds.model_depth = depth
        del drawn[:]
        trainer.stats.clear()
        mon.epoch(1)
        st = trainer.stats
        assert set(st) == {'ndb', 'ndb_over_k', 'jsd'} and [z.shape[0] for z in drawn] == [16, 16, 8]
        metric = mon._metric_obj
        assert metric.resolution == resolution and metric.holdout == 12
        check = pg.metrics.NDB(ds, k=5, holdout=12).fit()
        same_fit(metric, check)
        for z in drawn:
            check.feed(G.forward(z.cuda()))
        res = check.result()
        assert (st['ndb']['val'], st['ndb_over_k']['val'], st['jsd']['val']) == (res['ndb'], res['ndb_over_k'], res['jsd'])
        assert int(res['gen'].sum()) == 40
