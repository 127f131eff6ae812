"""The k-NN-ball tile kernel on the MI355X (csrc/prd.hip through ops.prd_kth_u8 / prd_ball_u8, metrics.PrecisionRecall,
plugins.PRDMonitor) against tests/prd_ref.py and against the numpy twin.  Integer arithmetic: EVERY comparison is ``==``.

Shapes are the smallest at which each part can go wrong.  A workgroup owns 128 x 128 pairs and walks D in chunks of 128 bytes: D = 16 is
one 16-byte piece of a chunk, 48 three, 192 a chunk and a half, 1024 eight chunks through both staging buffers; 3 x 256 x 256 = 196608
bytes of 255 against 0 put 65025 x 196608 > 2^31 into a distance and the shifted cross term below -2^31 (the int64 totals of the wide
instantiation).  Image counts: k + 1 (the minimum), 33 (one ragged tile), 128 (one full tile), 129 (the last candidate block holds one
column, which for row 128 is the diagonal: padding), 257 (three blocks; the diagonal falls in each)."""
import types

import numpy as np
import pytest
import torch

import prd_ref
from crops_ref import make_strips
from dataset_ref import make_stack

pytestmark = pytest.mark.gpu

SIZES = [(1, 4), (3, 4), (3, 8), (1, 32)]                      # D = 16, 48, 192, 1024
KS = [1, 3, 16]
COUNTS = [33, 128, 129, 257]                                   # and k + 1
BALL_SHAPES = [(1, 1), (5, 129), (129, 5), (128, 128), (257, 130)]
I64_MAX = np.iinfo(np.int64).max


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows(x):
    return x.reshape(len(x), -1)


_sets = {}


def data(C, r, n=257, seed=0):
    """The images of a size and the reference's distances between them, made once and shared (read only)."""
    key = (C, r, n, seed)
    if key not in _sets:
        x = prd_ref.images(n, C, r, seed=100 * r + C + seed)
        _sets[key] = (x, prd_ref.d2(x, x))
    return _sets[key]


def radii_of(dist, k):
    """prd_ref.radii on distances that are already there: the k-th smallest of every row without its diagonal element."""
    n = len(dist)
    return [sorted(int(dist[i, j]) for j in range(n) if j != i)[k - 1] for i in range(n)]


# ------------------------------------------------------------------------------------------------------------- prd_kth_u8
@pytest.mark.parametrize('C,r', SIZES)
def test_radii_against_the_reference_and_the_twin(pg, C, r):
    x, dist = data(C, r)
    assert radii_of(dist[:20, :20], 3) == prd_ref.radii(x[:20], 3).tolist()                 # (the shortcut is the reference)
    for k in KS:
        for N in [k + 1] + COUNTS:
            got = pg.ops.prd_kth_u8(dev(x[:N]), k)
            assert got.dtype == torch.int64 and tuple(got.shape) == (N,) and got.is_cuda
            assert got.cpu().tolist() == radii_of(dist[:N, :N], k), (C, r, k, N)
            assert got.cpu().tolist() == pg.metrics._radii_host(rows(x[:N]), k).tolist()
            assert torch.equal(got, pg.ops.prd_kth_u8(dev(x[:N]), k))                       # the same bits again


@pytest.mark.parametrize('N,k', [(129, 3), (257, 16), (2, 1), (130, 1)])
def test_candidate_blocks(pg, N, k):
    """What the tile kernel leaves for the second launch: per block of PRD_TILE columns the k smallest, ascending, INT64_MAX where the
    block has fewer than k columns other than the diagonal -- every element written (the buffer starts as -1)."""
    x = prd_ref.images(N, 3, 4, seed=5)
    blocks = (N + pg.ops.PRD_TILE - 1) // pg.ops.PRD_TILE
    cand = torch.full((N, blocks, k), -1, dtype=torch.int64, device='cuda')
    xd = dev(x)
    pg._lib.call('pg_prd_kth_u8', xd.data_ptr(), N, 48, k, cand.data_ptr(), pg.ops._stream())
    want = prd_ref.block_candidates(x, k, pg.ops.PRD_TILE)
    assert np.array_equal(cand.cpu().numpy(), want)
    if N == 129:
        assert want[128, 1].tolist() == [I64_MAX] * k and want[0, 1].tolist() == [int(prd_ref.d2(x[:1], x[128:])[0, 0])] + [I64_MAX] * (k - 1)


def test_a_duplicate_across_a_tile_boundary(pg):
    x = data(3, 4)[0].copy()
    x[200] = x[3]
    got = pg.ops.prd_kth_u8(dev(x), 1).cpu().tolist()
    assert got == prd_ref.radii(x, 1).tolist() and got[3] == got[200] == 0 and sum(1 for v in got if v == 0) == 2
    assert pg.ops.prd_kth_u8(dev(x), 2).cpu().tolist() == prd_ref.radii(x, 2).tolist()
    rad = dev(np.zeros(257, dtype=np.int64))
    a_cnt, a_hit, b_cnt, b_hit = pg.ops.prd_ball_u8(dev(x), dev(x), rad, rad)                # radius 0: itself, and the duplicate
    want = [2 if i in (3, 200) else 1 for i in range(257)]
    assert a_cnt.cpu().tolist() == a_hit.cpu().tolist() == b_cnt.cpu().tolist() == b_hit.cpu().tolist() == want


def test_widening_past_the_int32_accumulator(pg):
    """D = 3 x 256 x 256 = 196608 bytes of 255 against bytes of 0: the distance is 65025 x 196608 = 12 784 435 200 > 2^31 and the shifted
    cross term 127 x (-128) x 196608 < -2^31.  An accumulator that is not widened fails."""
    x = np.zeros((4, 3, 256, 256), dtype=np.uint8)
    x[0] = x[2] = 255
    far = 65025 * 196608
    assert far > 2 ** 31 and 127 * 128 * 196608 > 2 ** 31
    xd = dev(x)
    assert pg.ops.prd_kth_u8(xd, 1).cpu().tolist() == [0] * 4                              # the duplicates
    assert pg.ops.prd_kth_u8(xd, 2).cpu().tolist() == pg.ops.prd_kth_u8(xd, 3).cpu().tolist() == [far] * 4
    assert pg.metrics._radii_host(rows(x), 2).tolist() == [far] * 4
    for radius, near in ((far, 4), (far - 1, 2), (0, 2)):
        rad = dev(np.full(4, radius, dtype=np.int64))
        for out in pg.ops.prd_ball_u8(xd, xd, rad, rad):
            assert out.cpu().tolist() == [near] * 4
    y = prd_ref.images(3, 3, 256, seed=3)                                                    # ... and random bytes through the same path
    a_cnt, _, _, b_hit = pg.ops.prd_ball_u8(dev(y), xd, None, dev(prd_ref.d2(y[:1], x)[0]))
    want = prd_ref.ball_counts(y, x, None, prd_ref.d2(y[:1], x)[0])
    assert a_cnt.cpu().tolist() == want[0] and b_hit.cpu().tolist() == want[3] and want[0][0] == 4


@pytest.mark.parametrize('C', [4096, 4097, 4105])
def test_either_side_of_the_threshold_between_the_two_instantiations(pg, C):
    """D = 16 C: 65536 bytes are the last 512 chunks of the int32-only instantiation (loads one chunk ahead); 65552 and 65680 take the
    int64 totals and loads two chunks ahead through two register sets, with an odd (513, the last chunk one 16-byte piece) and an
    even number (514) of chunks."""
    x, y = prd_ref.images(6, C, 4, seed=C), prd_ref.images(3, C, 4, seed=C + 1)
    x[:, -1] = 255 - x[:, 0]                                                 # (the tail piece matters)
    assert pg.ops.prd_kth_u8(dev(x), 2).cpu().tolist() == prd_ref.radii(x, 2).tolist()
    dist = prd_ref.d2(y, x)
    check_ball(pg, y, x, np.sort(dist, axis=1)[:, 2].copy(), np.sort(dist, axis=0)[1].copy())


# ------------------------------------------------------------------------------------------------------------ prd_ball_u8
def check_ball(pg, a, b, rad_a, rad_b, dist=None):
    ra = None if rad_a is None else np.asarray(rad_a, dtype=np.int64)
    rb = None if rad_b is None else np.asarray(rad_b, dtype=np.int64)
    ad, bd = dev(a), dev(b)
    got = pg.ops.prd_ball_u8(ad, bd, None if ra is None else dev(ra), None if rb is None else dev(rb))
    again = pg.ops.prd_ball_u8(ad, bd, None if ra is None else dev(ra), None if rb is None else dev(rb))
    want = prd_ref.ball_counts(a, b, ra, rb)
    twin = pg.metrics._ball_host(rows(a), rows(b), ra, rb)
    for g, g2, w, t, n in zip(got, again, want, twin, (len(a), len(a), len(b), len(b))):
        assert (g is None) == (w is None) == (t is None)
        if g is not None:
            assert g.dtype == torch.int32 and tuple(g.shape) == (n,) and g.is_cuda
            assert g.cpu().tolist() == w == t.tolist() and torch.equal(g, g2)
    return want


@pytest.mark.parametrize('Na,Nb', BALL_SHAPES)
@pytest.mark.parametrize('C,r', [(3, 4), (3, 8)])
def test_ball_counts_against_the_reference_and_the_twin(pg, C, r, Na, Nb):
    a, b = data(C, r)[0][:Na], data(C, r, n=130, seed=1)[0][:Nb]
    dist = prd_ref.d2(a, b)
    rad_a = np.sort(dist, axis=1)[:, Nb // 2].copy()                          # every radius IS a distance of its row / column: each ball
    rad_b = np.sort(dist, axis=0)[Na // 2].copy()                             # has a probe on its boundary, which is inside
    both = check_ball(pg, a, b, rad_a, rad_b)
    assert all(v >= 1 for v in both[1] + both[3])
    only_a, only_b = check_ball(pg, a, b, rad_a, None), check_ball(pg, a, b, None, rad_b)
    assert only_a[1] == both[1] and only_a[2] == both[2] and only_b[0] == both[0] and only_b[3] == both[3]
    zero = check_ball(pg, a, b, np.zeros(Na), np.zeros(Nb))
    assert sum(zero[0]) == sum(zero[1]) == int((dist == 0).sum())
    one = int(dist[Na // 3, Nb // 2])                                         # every radius exactly one known distance
    known = check_ball(pg, a, b, np.full(Na, one), np.full(Nb, one))
    assert sum(known[0]) == sum(known[1]) == int((dist <= one).sum()) >= 1
    below = check_ball(pg, a, b, np.full(Na, one - 1), np.full(Nb, one - 1))
    assert sum(below[0]) < sum(known[0])
    every = check_ball(pg, a, b, np.full(Na, I64_MAX), np.full(Nb, I64_MAX))
    assert every[0] == every[1] == [Nb] * Na and every[2] == every[3] == [Na] * Nb


@pytest.mark.parametrize('C,r', [(1, 4), (1, 32)])
def test_ball_counts_at_the_other_sizes(pg, C, r):
    a, b = data(C, r)[0][:130], data(C, r, n=130, seed=1)[0][:67]
    dist = prd_ref.d2(a, b)
    check_ball(pg, a, b, np.sort(dist, axis=1)[:, 5].copy(), np.sort(dist, axis=0)[7].copy())


def test_argument_errors(pg):
    x = dev(prd_ref.images(8, 1, 4, seed=14))
    rad = torch.zeros(8, dtype=torch.int64, device='cuda')
    for k in (0, 17, 8, True, 2.5):                                          # k = 0, k = 17, N <= k
        with pytest.raises(ValueError):
            pg.ops.prd_kth_u8(x, k)
    with pytest.raises(ValueError):
        pg.ops.prd_kth_u8(dev(np.zeros((8, 1, 2, 2), dtype=np.uint8)), 1)    # D = 4
    with pytest.raises(ValueError):
        pg.ops.prd_kth_u8(x.cpu(), 1)
    with pytest.raises(ValueError):
        pg.ops.prd_ball_u8(x, x)                                             # no radii
    with pytest.raises(ValueError):
        pg.ops.prd_ball_u8(x, dev(prd_ref.images(8, 3, 4, seed=1)), rad, rad)        # mismatched shapes
    with pytest.raises(ValueError):
        pg.ops.prd_ball_u8(x, x[:5], rad, rad)                               # rad_b of another length
    with pytest.raises(ValueError):
        pg.ops.prd_ball_u8(x, x, rad.int(), None)
    with pytest.raises(ValueError):
        pg.ops.prd_ball_u8(x, x, rad.cpu(), None)
    cand = torch.full((8, 1, 16), -1, dtype=torch.int64, device='cuda')
    out = [torch.full((8,), -1, dtype=torch.int32, device='cuda') for _ in range(4)]
    s = pg.ops._stream()
    xp, rp, cp = x.data_ptr(), rad.data_ptr(), cand.data_ptr()
    o = [t.data_ptr() for t in out]
    for name, args, err in (('pg_prd_kth_u8', (xp, 8, 16, 0, cp, s), 'PG_E_ARG'),
                            ('pg_prd_kth_u8', (xp, 8, 16, 17, cp, s), 'PG_E_ARG'),
                            ('pg_prd_kth_u8', (xp, 8, 16, 8, cp, s), 'PG_E_ARG'),                        # N <= k
                            ('pg_prd_kth_u8', (xp, 3, 16, 3, cp, s), 'PG_E_ARG'),
                            ('pg_prd_kth_u8', (None, 8, 16, 1, cp, s), 'PG_E_ARG'),
                            ('pg_prd_kth_u8', (xp, 4, 24, 1, cp, s), 'PG_E_ALIGN'),                      # D % 16
                            ('pg_prd_kth_u8', (xp + 8, 4, 16, 1, cp, s), 'PG_E_ALIGN'),
                            ('pg_prd_ball_u8', (xp, 8, xp, 8, 16, None, None, o[0], o[1], o[2], o[3], s), 'PG_E_ARG'),
                            ('pg_prd_ball_u8', (xp, 8, xp, 8, 16, rp, None, None, o[1], None, None, s), 'PG_E_ARG'),   # rad_a without b_cnt
                            ('pg_prd_ball_u8', (xp, 8, xp, 8, 16, None, rp, None, None, None, o[3], s), 'PG_E_ARG'),   # rad_b without a_cnt
                            ('pg_prd_ball_u8', (xp, 0, xp, 8, 16, rp, rp, o[0], o[1], o[2], o[3], s), 'PG_E_ARG'),
                            ('pg_prd_ball_u8', (xp, 4, xp, 4, 24, rp, rp, o[0], o[1], o[2], o[3], s), 'PG_E_ALIGN'),
                            ('pg_prd_ball_u8', (xp, 4, xp + 8, 4, 16, rp, rp, o[0], o[1], o[2], o[3], s), 'PG_E_ALIGN'),
                            ('pg_prd_ball_u8', (xp, 4, xp, 4, 16, rp + 4, rp, o[0], o[1], o[2], o[3], s), 'PG_E_ALIGN')):
        with pytest.raises(RuntimeError, match=err):
            pg._lib.call(name, *args)
    torch.cuda.synchronize()
    assert int((cand != -1).sum()) == 0 and all(int((t != -1).sum()) == 0 for t in out)     # refused before any launch or memset
    # a skipped pair of outputs is not touched, and its pointers may be NULL
    pg._lib.call('pg_prd_ball_u8', xp, 8, xp, 8, 16, None, rp, o[0], None, None, o[3], s)
    assert out[0].cpu().tolist() == out[3].cpu().tolist() == [1] * 8 and int((out[1] != -1).sum()) == int((out[2] != -1).sum()) == 0


# ---------------------------------------------------------------------------------------------------- metrics.PrecisionRecall
def same_result(a, b):
    assert a == b and set(a) == {'precision', 'recall', 'density', 'coverage', 'num_real', 'num_fake', 'k'}


def test_identical_sets_and_two_clusters_on_the_device(pg):
    x = prd_ref.images(40, 3, 8, seed=9)
    for k in (1, 3):
        m = pg.metrics.PrecisionRecall(dev(x), k=k).fit()
        m.feed_u8(dev(x))
        res = m.result()
        assert (res['precision'], res['recall'], res['coverage']) == (1.0, 1.0, 1.0) and res['density'] == (k + 1) / float(k)
    reals, fakes = prd_ref.two_clusters()
    rad_r, rad_f = pg.ops.prd_kth_u8(dev(reals), 3), pg.ops.prd_kth_u8(dev(fakes), 3)
    assert rad_r.cpu().tolist() == prd_ref.radii(reals, 3).tolist()
    _, _, b_cnt, b_hit = pg.ops.prd_ball_u8(dev(fakes), dev(reals), rad_f, rad_r)
    assert b_cnt[40:].cpu().tolist() == [0] * 24 and b_hit[40:].cpu().tolist() == [0] * 24
    m = pg.metrics.PrecisionRecall(dev(reals), k=3).fit()
    m.feed_u8(dev(fakes))
    twin = pg.metrics.PrecisionRecall(torch.from_numpy(reals), k=3, device='cpu').fit()
    twin.feed_u8(torch.from_numpy(fakes))
    same_result(m.result(), twin.result())
    assert m.result()['recall'] <= 40 / 64.0 and m.result()['coverage'] <= 40 / 64.0
    want = prd_ref.prd(reals[m.indices.numpy()], fakes, 3)
    assert {n: m.result()[n] for n in want} == want


@pytest.mark.parametrize('pyramid', ['chain', 'direct'])
def test_metric_over_a_device_dataset(pg, pyramid):
    stack = make_stack(150, 3, 32, seed=4)
    ds = pg.DeviceImageDataset(stack, pyramid=pyramid, model_initial_depth=1)                # 8x8: two levels below the source
    twin_ds = pg.DeviceImageDataset(stack, pyramid=pyramid, model_initial_depth=1, device='cpu')
    samples = torch.rand(140, 3, 8, 8, generator=torch.Generator().manual_seed(3)) * 2 - 1
    near = pg.ops.real_batch_u8(ds.level_stack(), torch.arange(0, 40, device='cuda'))        # training images as G would emit them
    samples[:40] = (near + 0.02).clamp(-1, 1).cpu()
    for kw in (dict(k=3), dict(k=2, num_real=131, seed=4), dict(k=3, max_resolution=4)):
        m = pg.metrics.PrecisionRecall(ds, **kw).fit()
        twin = pg.metrics.PrecisionRecall(twin_ds, device='cpu', **kw).fit()
        assert m.reals.is_cuda and m.radii.is_cuda and m.resolution == 8
        assert torch.equal(m.reals.cpu(), twin.reals) and torch.equal(m.radii.cpu(), twin.radii) and torch.equal(m.indices, twin.indices)
        for s in range(0, 140, 48):
            m.feed(samples[s:s + 48].cuda())
            twin.feed(samples[s:s + 48])
        same_result(m.result(), twin.result())
        assert m.result()['num_fake'] == 140
        if 'max_resolution' not in kw:                                                       # ... and the reference on the same levels
            want = prd_ref.prd(twin_ds.level_stack().numpy()[m.indices.numpy()], pg.metrics._quantise_host(samples.numpy(), (-1, 1)), kw['k'])
            assert {n: m.result()[n] for n in want} == want
    ds.model_depth = twin_ds.model_depth = 2                                                 # the fit follows the stage
    m.fit(), twin.fit()
    assert m.resolution == 16 and tuple(m.reals.shape) == (150, 3, 4, 4) and torch.equal(m.radii.cpu(), twin.radii)


def test_metric_over_a_strip_dataset(pg):
    strips = make_strips(2, 16, widths=(5, 3, 4), extra=7, seed=6)
    ds = pg.DeviceStripDataset(strips, model_initial_depth=2, device='cuda')
    twin_ds = pg.DeviceStripDataset(strips, model_initial_depth=2, device='cpu')
    level = ds.level_stack()
    assert tuple(level.shape) == (12, 2, 16, 16) and torch.equal(level.cpu(), twin_ds.level_stack())
    m = pg.metrics.PrecisionRecall(ds, k=2).fit()
    twin = pg.metrics.PrecisionRecall(twin_ds, k=2, device='cpu').fit()
    assert torch.equal(m.radii.cpu(), twin.radii) and m.radii.cpu().tolist() == prd_ref.radii(level.cpu().numpy()[m.indices.numpy()], 2).tolist()
    fakes = level[:7].clone()
    fakes[:, :, 3, 3] ^= 1
    m.feed_u8(fakes)
    twin.feed_u8(fakes.cpu())
    same_result(m.result(), twin.result())
    assert m.result()['precision'] == 1.0


# ---------------------------------------------------------------------------------------------------------- plugins.PRDMonitor
def test_monitor_in_a_two_tick_trainer_run_at_4x4(pg):
    torch.manual_seed(3)
    shape = (1, 3, 16, 16)
    kw = dict(fmap_base=64, fmap_max=16)
    G, D = pg.Generator(shape, latent_size=16, **kw).cuda(), pg.Discriminator(shape, **kw).cuda()
    opt_g = pg.FusedAdam(G.parameters(), 0.001, betas=(0.0, 0.99))
    opt_d = pg.FusedAdam(D.parameters(), 0.001, betas=(0.0, 0.99))
    ds = pg.DeviceImageDataset(make_stack(24, 3, 16, seed=7), seed=6)

    def rlg(n):
        g = torch.Generator().manual_seed(5)
        return lambda: torch.randn(n, 16, generator=g)

    tr = pg.Trainer(D, G, pg.wgan_gp_D_loss, pg.wgan_gp_G_loss, opt_d, opt_g, ds, None, None)
    tr.register_plugin(pg.DepthManager(ds.loader, rlg, 2, minibatch_default=4, minibatch_overrides={}, tick_kimg_default=0.008,
                                       tick_kimg_overrides={}, lod_training_nimg=1000, lod_transition_nimg=1000))
    g = torch.Generator().manual_seed(9)
    drawn, seen = [], []

    def sample_fn(n):
        drawn.append(n)
        return torch.randn(n, 16, generator=g)

    mon = pg.PRDMonitor(ds, sample_fn, num_samples=20, minibatch=8, k=3, prd_ticks=1)
    tr.register_plugin(mon)

    class Record(pg.Plugin):
        def __init__(self):
            super(Record, self).__init__([(1, 'epoch')])

        def register(self, trainer):
            pass

        def epoch(self, tick):
            seen.append({n: tr.stats[n]['val'] for n in ('precision', 'recall', 'density', 'coverage')})

    tr.register_plugin(Record())
    tr.run(0.016)                                                            # two ticks of 8 images at 4x4, then the end
    torch.cuda.synchronize()
    assert tr.cur_tick == 2 and G.depth == 0 and len(seen) == 2 and drawn == [8, 8, 4] * 3
    metric = mon._metric_obj
    assert metric.resolution == 4 and tuple(metric.reals.shape) == (24, 3, 4, 4) and metric.result()['num_fake'] == 20
    for st in seen + [{n: tr.stats[n]['val'] for n in seen[0]}]:
        assert all(0.0 <= st[n] <= 1.0 for n in ('precision', 'recall', 'coverage')) and 0.0 <= st['density'] <= 24 / 3.0
    assert {n: tr.stats[n]['val'] for n in seen[0]} == {n: metric.result()[n] for n in seen[0]}
    assert metric.radii.cpu().tolist() == prd_ref.radii(ds.level_stack().cpu().numpy()[metric.indices.numpy()], 3).tolist()
