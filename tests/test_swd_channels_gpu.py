"""The sliced Wasserstein metric for 1, 2 and 4 channels on the MI355X (include/pggan_hip_swd.h through ops.swd_gather_c /
swd_normalize_c_ / swd_project_c, metrics.ChannelSlicedWasserstein, plugins.SWDMonitor) against its torch-CPU statement
tests/swd_ref.py, which is written over the channel count of its input.  The bounds are those of tests/test_swd_gpu.py -- the
arithmetic per channel is unchanged; the projection's is scaled by the number of accumulated terms for 196 -- and three channels through
the new entry points equal the old ones bit for bit.  UNPINNED for C != 3: this project's extension of the paper's 7x7x3 descriptor."""
import types

import numpy as np
import pytest
import torch

import swd_ref

pytestmark = pytest.mark.gpu
CHANNELS = [1, 2, 4]
SCALE = [0.5, 2.0, 1.0, 3.0]
MEAN = [3.0, -1.0, 0.1, -4.0]


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit_dirs(seed, width, K):
    d = torch.randn(width, K, generator=_gen(seed), dtype=torch.float64)
    return d / d.pow(2).sum(dim=0, keepdim=True).sqrt()


def _centres(S, N, P, seed):
    """Random centres with four of them pinned to the corners of [3, S-4]^2 (rows 0, 4, 7 and N*P - 1)."""
    c = torch.randint(3, S - 3, (N * P, 2), generator=_gen(seed), dtype=torch.int32)
    c[0], c[4], c[7], c[N * P - 1] = torch.tensor([[3, 3], [S - 4, 3], [3, S - 4], [S - 4, S - 4]], dtype=torch.int32)
    return c


def _scaled_desc(M, C, seed):
    """[M,C,7,7]: every channel with a mean and a scale of its own"""
    return torch.randn(M, C, 7, 7, generator=_gen(seed)) * torch.tensor(SCALE[:C]).view(1, C, 1, 1) + torch.tensor(MEAN[:C]).view(1, C, 1, 1)


# ------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize('S', [16, 32])
@pytest.mark.parametrize('C', CHANNELS)
def test_gather(pg, C, S):
    N, P, off = 3, 5, 4
    W = 49 * C
    level = torch.randn(N, C, S, S, generator=_gen(S + C))
    centres = _centres(S, N, P, S + 1)
    rows = off + N * P + 3
    out = torch.full((rows, W), -7.5).cuda()
    pg.ops.swd_gather_c(level.cuda(), centres.cuda(), P, out, off)
    out = out.cpu()
    assert torch.equal(out[off:off + N * P], swd_ref.descriptors(level, centres, P).reshape(N * P, W))
    assert bool((out[:off] == -7.5).all()) and bool((out[off + N * P:] == -7.5).all())
    for other in sorted({49, 98, 147, 196, 245, 50} - {W}):                                                        # another width
        with pytest.raises(ValueError):
            pg.ops.swd_gather_c(level.cuda(), centres.cuda(), P, torch.empty(rows, other).cuda(), 0)
    with pytest.raises(ValueError):
        pg.ops.swd_gather_c(torch.zeros(N, 5, S, S).cuda(), centres.cuda(), P, torch.empty(rows, 245).cuda(), 0)   # C = 5
    with pytest.raises(ValueError):
        pg.ops.swd_gather_c(level.cuda(), centres.cuda(), P, torch.empty(rows, W).cuda(), rows - N * P + 1)        # rows past the end
    for j, xy in ((2, (2, 5)), (9, (5, S - 3)), (11, (S - 3, 3)), (0, (3, -1))):                                   # a centre out of [3, S-4]
        bad = centres.clone()
        bad[j] = torch.tensor(xy, dtype=torch.int32)
        with pytest.raises(ValueError):
            pg.ops.swd_gather_c(level.cuda(), bad.cuda(), P, torch.empty(rows, W).cuda(), 0)


def test_entry_points_refuse_a_channel_count_outside_1_to_4(pg):
    """PG_E_ARG from the library itself, before any launch (the wrappers never pass such a count on)."""
    lib = pg._lib.load()
    buf = torch.zeros(4096, device='cuda')
    part = torch.zeros(pg.ops.SWD_REDUCE_BLOCKS * 10, device='cuda', dtype=torch.float64)
    cen = torch.full((1, 2), 3, dtype=torch.int32, device='cuda')
    E_ARG = pg._lib.CONSTANTS['PG_E_ARG']
    for C in (0, 5, -1):
        assert lib.pg_swd_gather_c(buf.data_ptr(), cen.data_ptr(), buf.data_ptr(), 1, 1, C, 16, 0, 1, None) == E_ARG
        assert lib.pg_swd_channel_stats_c(buf.data_ptr(), 1, C, part.data_ptr(), buf.data_ptr(), None) == E_ARG
        assert lib.pg_swd_normalize_c(buf.data_ptr(), 1, C, buf.data_ptr(), None) == E_ARG
        assert lib.pg_swd_project_c(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, C, 1, None) == E_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- normalise
@pytest.mark.parametrize('M', [7, 1000])
@pytest.mark.parametrize('C', CHANNELS)
def test_normalize(pg, C, M):
    desc = _scaled_desc(M, C, M + C)
    ref = swd_ref.normalize(desc.double())
    got = pg.ops.swd_normalize_c_(desc.reshape(M, 49 * C).contiguous().cuda()).cpu().double()
    err = float((got - ref).abs().max())
    mean = got.view(M, C, 49).mean(dim=(0, 2))
    std = got.view(M, C, 49).std(dim=(0, 2), unbiased=False)
    print('swd_normalize_c_ C=%d M=%d: max abs err %.3e, |mean| %.3e, |std-1| %.3e'
          % (C, M, err, float(mean.abs().max()), float((std - 1).abs().max())))
    assert err <= 1e-5
    assert float(mean.abs().max()) <= 1e-5
    assert float((std - 1).abs().max()) <= 1e-5
    with pytest.raises(ValueError):
        pg.ops.swd_normalize_c_(torch.zeros(M, 49 * C + 1).cuda())
    with pytest.raises(ValueError):
        pg.ops.swd_normalize_c_(torch.zeros(M, 245).cuda())


# ------------------------------------------------------------------------------------------------- projection
PROJECT_MAX = {}


@pytest.mark.parametrize('K', [1, 64, 128, 160])                         # 160: a second, partial block of directions
@pytest.mark.parametrize('M', [1, 37, 1000])                             # 1000: 7 full workgroups and a ragged one of 104 rows
@pytest.mark.parametrize('C', CHANNELS)
def test_project(pg, C, M, K):
    W = 49 * C
    desc = torch.randn(M, W, generator=_gen(1000 * M + K + C))            # what normalised descriptors look like: zero mean, unit variance
    dirs = _unit_dirs(K + C, W, K).float().contiguous()
    got = pg.ops.swd_project_c(desc.cuda(), dirs.cuda())
    assert tuple(got.shape) == (K, M) and got.is_contiguous()
    ref = (desc.double() @ dirs.double()).t()
    err = float((got.cpu().double() - ref).abs().max())
    PROJECT_MAX[C] = max(PROJECT_MAX.get(C, 0.0), err)
    print('swd_project_c C=%d M=%d K=%d: max abs err %.3e (largest for C=%d so far %.3e)' % (C, M, K, err, C, PROJECT_MAX[C]))
    assert err <= (2e-5 if W <= 147 else 2e-5 * 196 / 147)               # the three-channel bound, scaled by the accumulated terms


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_project_from_a_base_that_is_not_16_byte_aligned(pg, C):
    """Full workgroups are copied into LDS sixteen bytes at a time when their first row allows it.  Rows 1.. of a tensor start 49 C
    floats behind an aligned base: a multiple of 16 bytes only for C = 4.  Either way the result is that of an aligned copy, bit for bit."""
    W, M, K = 49 * C, 300, 64                                             # two full workgroups and a ragged one
    big = torch.randn(M + 1, W, generator=_gen(40 + C)).cuda()
    dirs = _unit_dirs(50 + C, W, K).float().contiguous().cuda()
    view = big[1:]
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (C == 4)
    got, want = pg.ops.swd_project_c(view, dirs), pg.ops.swd_project_c(view.clone(), dirs)
    assert torch.equal(got, want)
    ref = (view.cpu().double() @ dirs.cpu().double()).t()
    assert float((got.cpu().double() - ref).abs().max()) <= (2e-5 if W <= 147 else 2e-5 * 196 / 147)


def test_project_argument_errors(pg):
    d = torch.zeros(4, 98).cuda()
    with pytest.raises(ValueError):
        pg.ops.swd_project_c(d, torch.zeros(147, 8).cuda())               # 2 channels against 3
    with pytest.raises(ValueError):
        pg.ops.swd_project_c(torch.zeros(4, 100).cuda(), torch.zeros(100, 8).cuda())
    with pytest.raises(ValueError):
        pg.ops.swd_project_c(d, torch.zeros(98, 8).cuda(), out=torch.zeros(4, 8).cuda())      # out must be [K,M]
    with pytest.raises(ValueError):
        pg.ops.swd_gather(torch.zeros(2, 1, 16, 16).cuda(), torch.full((2, 2), 3, dtype=torch.int32).cuda(), 1, torch.zeros(2, 147).cuda(), 0)


# ------------------------------------------------------------------------------------------------- C = 3: the old path's bits
def test_three_channels_equal_the_old_entry_points_bit_for_bit(pg):
    N, P, S, K = 8, 125, 32, 128                                          # M = 1000 descriptors
    M = N * P
    level = (torch.randn(N, 3, S, S, generator=_gen(5)) * torch.tensor(SCALE[:3]).view(1, 3, 1, 1) + torch.tensor(MEAN[:3]).view(1, 3, 1, 1)).cuda()
    centres = _centres(S, N, P, 6).cuda()
    old = pg.ops.swd_gather(level, centres, P, torch.full((M, 147), -7.5).cuda(), 0)
    new = pg.ops.swd_gather_c(level, centres, P, torch.full((M, 147), -7.5).cuda(), 0)
    assert torch.equal(old, new) and not bool((new == -7.5).any())
    pg.ops.swd_normalize_(old)
    pg.ops.swd_normalize_c_(new)
    assert torch.equal(old, new)
    assert float(new.view(M, 3, 49).double().mean(dim=(0, 2)).abs().max()) <= 1e-5       # (and both did normalise)
    dirs = _unit_dirs(K, 147, K).float().contiguous().cuda()
    a, b = pg.ops.swd_project(old, dirs), pg.ops.swd_project_c(new, dirs)
    assert torch.equal(a, b) and float(b.abs().max()) > 1.0
    # ... and on the inputs of the per-kernel tests
    desc = _scaled_desc(M, 3, 1000).reshape(M, 147).contiguous()
    assert torch.equal(pg.ops.swd_normalize_(desc.clone().cuda()), pg.ops.swd_normalize_c_(desc.clone().cuda()))
    desc = torch.randn(M, 147, generator=_gen(1000 * M + K)).cuda()
    assert torch.equal(pg.ops.swd_project(desc, dirs), pg.ops.swd_project_c(desc, dirs))


# ------------------------------------------------------------------------------------------------- end to end
def _smooth(g, C, n=16):
    """8x8 Gaussian noise repeated x4 in both directions, plus 0.3 * noise"""
    low = torch.randn(n, C, 8, 8, generator=g)
    return (low.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3) + 0.3 * torch.randn(n, C, 32, 32, generator=g)).contiguous()


def make_sets(C):
    g = _gen(11 + C)
    return {'A': _smooth(g, C), 'B': _smooth(g, C), 'noise': torch.randn(16, C, 32, 32, generator=g)}


KW = dict(patches_per_image=32, dir_repeats=4, dirs_per_repeat=64)


@pytest.fixture(scope='module')
def e2e(pg):
    """Per C: the sets and one metric object, made once."""
    cache = {}

    def get(C):
        if C not in cache:
            cache[C] = (make_sets(C), pg.metrics.ChannelSlicedWasserstein(32, 16, C, seed=1, **KW))
        return cache[C]
    return get


def _run_metric(metric, real, fake, minibatch=5):
    metric.reset()
    for s in range(0, real.shape[0], minibatch):
        metric.feed_real(real[s:s + minibatch].contiguous().cuda())
        metric.feed_fake(fake[s:s + minibatch].contiguous().cuda())
    return metric.result()


@pytest.mark.parametrize('pair', [('A', 'B'), ('A', 'noise'), ('A', 'A')])
@pytest.mark.parametrize('C', CHANNELS)
def test_metric_end_to_end(pg, e2e, C, pair):
    sets, m = e2e(C)
    assert m.levels == [32, 16] and m.num_channels == C and tuple(m.directions.shape) == (4, 49 * C, 64)
    assert float((m.directions.double().pow(2).sum(dim=1) - 1).abs().max()) < 1e-6
    for c, s in zip(m.centres, m.levels):
        assert tuple(c.shape) == (16 * 32, 2) and c.dtype == torch.int32 and int(c.min()) >= 3 and int(c.max()) <= s - 4
    real, fake = sets[pair[0]], sets[pair[1]]
    got = _run_metric(m, real, fake)
    ref = swd_ref.swd(real.double(), fake.double(), m.centres, m.directions.double(), 32)
    assert got['levels'] == [32, 16]
    for lv, a, b in zip(got['levels'], got['swd'], ref['swd']):
        print('SWD C=%d %s/%s level %d: device %.6f  fp64 %.6f  |diff| %.3e' % (C, pair[0], pair[1], lv, a, b, abs(a - b)))
    for a, b in zip(got['swd'] + [got['mean']], ref['swd'] + [ref['mean']]):
        assert abs(a - b) <= 1e-3
    if pair[0] == pair[1]:
        assert got['swd'] == [0.0, 0.0] and got['mean'] == 0.0
    else:
        assert min(got['swd']) > 10.0                                     # (different sets are whole units apart)


@pytest.mark.parametrize('C', CHANNELS)
def test_metric_is_a_function_of_its_seed(pg, e2e, C):
    sets, m = e2e(C)
    a, b = sets['A'], sets['B']
    r1 = _run_metric(m, a, b)
    r2 = _run_metric(pg.metrics.ChannelSlicedWasserstein(32, 16, C, seed=1, **KW), a, b, minibatch=16)
    r3 = _run_metric(pg.metrics.ChannelSlicedWasserstein(32, 16, C, seed=2, **KW), a, b)
    assert r1 == r2                                                       # bit for bit, whatever the split into minibatches
    assert r1['swd'] != r3['swd']


def test_three_channel_metric_equals_sliced_wasserstein(pg):
    sets = make_sets(3)
    new = pg.metrics.ChannelSlicedWasserstein(32, 16, 3, seed=1, **KW)
    old = pg.metrics.SlicedWasserstein(32, 16, seed=1, **KW)
    assert torch.equal(new.directions, old.directions) and len(new.centres) == len(old.centres) == 2
    assert all(torch.equal(a, b) for a, b in zip(new.centres, old.centres))
    for pair in (('A', 'B'), ('A', 'noise')):
        r_new, r_old = _run_metric(new, sets[pair[0]], sets[pair[1]]), _run_metric(old, sets[pair[0]], sets[pair[1]])
        assert r_new == r_old and min(r_new['swd']) > 10.0


@pytest.mark.parametrize('C', CHANNELS)
def test_metric_feed_errors(pg, C):
    m = pg.metrics.ChannelSlicedWasserstein(32, 4, C, patches_per_image=4, dir_repeats=1, dirs_per_repeat=8)
    a = make_sets(C)['A'].cuda()
    with pytest.raises(ValueError):
        m.feed_real(torch.zeros(2, 3 if C != 3 else 1, 32, 32).cuda())    # another channel count
    with pytest.raises(ValueError):
        m.feed_real(torch.zeros(2, C + 1, 32, 32).cuda())
    with pytest.raises(ValueError):
        m.feed_real(a[:2, :, :16, :16].contiguous())                      # another resolution
    with pytest.raises(ValueError):
        m.feed_real(a[:5])                                                # more than num_images
    m.feed_real(a[:4])
    with pytest.raises(RuntimeError):
        m.result()                                                        # no fake images yet


# ------------------------------------------------------------------------------------------------- the plugin
def test_swd_monitor_measures_a_two_channel_network(pg):
    torch.manual_seed(3)
    G = pg.Generator((1, 2, 16, 16), latent_size=32, fmap_base=128, fmap_max=32)
    G.to('cuda')
    G.depth, G.alpha = 2, 1.0
    assert G.num_channels == 2
    g = _gen(21)
    reals, fakes = [], []

    def real_batch_fn(n):
        reals.append(torch.randn(n, 2, 16, 16, generator=g).cuda())
        return reals[-1]

    def forward(z):
        fakes.append(G.forward(z).clone())                                # (a later pass may reuse the output buffer)
        return fakes[-1]

    def run(real_fn):
        trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=0, G=types.SimpleNamespace(depth=2, num_channels=2, forward=forward))
        mon = pg.SWDMonitor(real_fn, lambda n: torch.randn(n, 32, generator=g), num_images=8, minibatch=3, swd_ticks=1,
                            patches_per_image=8)
        mon.register(trainer)
        mon.epoch(1)
        return trainer.stats

    st = run(real_batch_fn)
    assert [r.shape[0] for r in reals] == [3, 3, 2] and [tuple(f.shape) for f in fakes] == [(3, 2, 16, 16), (3, 2, 16, 16), (2, 2, 16, 16)]
    direct = pg.metrics.ChannelSlicedWasserstein(16, 8, 2, patches_per_image=8)
    direct.feed_real(torch.cat(reals))
    direct.feed_fake(torch.cat(fakes))
    res = direct.result()
    assert st['swd']['val'] == res['mean'] and st['swd_16']['val'] == res['swd'][0] and res['mean'] > 0
    assert st['swd']['log_name'] == 'swd' and st['swd']['log_epoch_fields'][0].format(**st['swd'])
    assert set(st) == {'swd', 'swd_16'}

    # the sound path: reals from a two-channel device dataset's metric batches
    stack = torch.randint(0, 256, (12, 2, 16, 16), generator=_gen(22), dtype=torch.uint8).numpy()
    ds = pg.DeviceImageDataset(stack, model_initial_depth=2, two_channel=True)
    f = ds.metric_batches()
    seen = []

    def dataset_batch_fn(n):
        seen.append(f(n).clone())
        return seen[-1]

    del fakes[:]
    st = run(dataset_batch_fn)
    assert [tuple(b.shape) for b in seen] == [(3, 2, 16, 16), (3, 2, 16, 16), (2, 2, 16, 16)] and all(b.is_cuda for b in seen)
    direct.reset()
    direct.feed_real(torch.cat(seen))
    direct.feed_fake(torch.cat(fakes))
    res = direct.result()
    assert set(st) == {'swd', 'swd_16'} and st['swd']['val'] == res['mean'] and st['swd_16']['val'] == res['swd'][0]
    assert np.isfinite(res['mean']) and res['mean'] > 0
