"""The sliced Wasserstein metric on the MI355X (csrc/swd.hip through ops.py, metrics.SlicedWasserstein, plugins.SWDMonitor) against
its torch-CPU statement tests/swd_ref.py.  Shapes are the smallest at which each kernel can still go wrong; every bound is the one
the definition gives (fp32 rounding of a 25-term filter, fp64 references for the reductions, bit equality for gather and sort)."""
import types

import pytest
import torch

import swd_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit_dirs(seed, R, K):
    d = torch.randn(R, 147, K, generator=_gen(seed), dtype=torch.float64)
    return d / d.pow(2).sum(dim=1, keepdim=True).sqrt()


# ------------------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize('shape', [(2, 3, 16, 16), (2, 3, 32, 32), (1, 3, 128, 128)])
def test_lap_pyramid(pg, shape):
    x = torch.rand(shape, generator=_gen(shape[-1]), dtype=torch.float32) * 2 - 1
    got = pg.ops.lap_pyramid(x.cuda())
    ref = swd_ref.lap_pyramid(x)
    assert [tuple(l.shape) for l in got] == [tuple(l.shape) for l in ref]
    assert len(got) == {16: 1, 32: 2, 128: 4}[shape[-1]]
    for g, r in zip(got, ref):
        err = float((g.cpu() - r).abs().max())
        print('lap_pyramid %s level %d: max abs err %.3e' % (shape, r.shape[-1], err))
        assert err <= 2e-6
    if shape[-1] == 16:
        assert torch.equal(got[0].cpu(), x)                              # one level: the identity path


def test_lap_pyramid_argument_errors(pg):
    for bad in (torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 24, 24), torch.zeros(2, 3, 32, 16), torch.zeros(3, 32, 32)):
        with pytest.raises(ValueError):
            pg.ops.lap_pyramid(bad.cuda())
    with pytest.raises(ValueError):
        pg.ops.lap_pyramid(torch.zeros(2, 3, 32, 32))                    # not on the device


# ------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize('S', [16, 32])
def test_swd_gather(pg, S):
    N, P, off = 3, 5, 4
    level = torch.randn(N, 3, S, S, generator=_gen(S))
    centres = torch.randint(3, S - 3, (N * P, 2), generator=_gen(S + 1), dtype=torch.int32)
    centres[0], centres[4], centres[7], centres[14] = torch.tensor([[3, 3], [S - 4, 3], [3, S - 4], [S - 4, S - 4]], dtype=torch.int32)
    rows = off + N * P + 3
    out = torch.full((rows, 147), -7.5).cuda()
    pg.ops.swd_gather(level.cuda(), centres.cuda(), P, out, off)
    out = out.cpu()
    assert torch.equal(out[off:off + N * P], swd_ref.descriptors(level, centres, P).reshape(N * P, 147))
    assert bool((out[:off] == -7.5).all()) and bool((out[off + N * P:] == -7.5).all())
    with pytest.raises(ValueError):
        pg.ops.swd_gather(level.cuda(), centres.cuda(), P, torch.empty(rows, 147).cuda(), rows - N * P + 1)      # rows past the end
    with pytest.raises(ValueError):
        pg.ops.swd_gather(level.cuda(), centres.long().cuda(), P, torch.empty(rows, 147).cuda(), 0)   # not int32
    with pytest.raises(ValueError):
        pg.ops.swd_gather(level[:, :1].contiguous().cuda(), centres.cuda(), P, torch.empty(rows, 147).cuda(), 0)   # C = 1
    for j, xy in ((2, (2, 5)), (9, (5, S - 3)), (11, (S - 3, 3)), (0, (3, -1))):                                   # a centre out of [3, S-4]
        bad = centres.clone()
        bad[j] = torch.tensor(xy, dtype=torch.int32)
        with pytest.raises(ValueError):
            pg.ops.swd_gather(level.cuda(), bad.cuda(), P, torch.empty(rows, 147).cuda(), 0)


# ------------------------------------------------------------------------------------------------- normalise
@pytest.mark.parametrize('M', [7, 1000])
def test_swd_normalize(pg, M):
    g = _gen(M)
    desc = torch.randn(M, 3, 7, 7, generator=g) * torch.tensor([0.5, 2.0, 1.0]).view(1, 3, 1, 1) + torch.tensor([3.0, -1.0, 0.1]).view(1, 3, 1, 1)
    ref = swd_ref.normalize(desc.double())
    got = pg.ops.swd_normalize_(desc.reshape(M, 147).contiguous().cuda()).cpu().double()
    err = float((got - ref).abs().max())
    mean = got.view(M, 3, 49).mean(dim=(0, 2))
    std = got.view(M, 3, 49).std(dim=(0, 2), unbiased=False)
    print('swd_normalize_ M=%d: max abs err %.3e, |mean| %.3e, |std-1| %.3e' % (M, err, float(mean.abs().max()), float((std - 1).abs().max())))
    assert err <= 1e-5
    assert float(mean.abs().max()) <= 1e-5
    assert float((std - 1).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------- projection
@pytest.mark.parametrize('K', [1, 64, 128])
@pytest.mark.parametrize('M', [1, 37, 1000])
def test_swd_project(pg, M, K):
    g = _gen(1000 * M + K)
    desc = torch.randn(M, 147, generator=g)                               # what normalised descriptors look like: zero mean, unit variance
    dirs = _unit_dirs(K, 1, K)[0].float().contiguous()
    got = pg.ops.swd_project(desc.cuda(), dirs.cuda())
    assert tuple(got.shape) == (K, M) and got.is_contiguous()
    ref = (desc.double() @ dirs.double()).t()
    err = float((got.cpu().double() - ref).abs().max())
    print('swd_project M=%d K=%d: max abs err %.3e' % (M, K, err))
    assert err <= 2e-5


# ------------------------------------------------------------------------------------------------- sort
def _sort_rows(kind, K, M, seed):
    g = _gen(seed)
    if kind == 'normal':
        return torch.randn(K, M, generator=g)
    if kind == 'equal':
        return torch.full((K, M), -1.25)
    if kind == 'descending':
        return torch.randn(K, M, generator=g).sort(dim=1, descending=True)[0].contiguous()
    pool = torch.tensor([-3.5, -1.0, -1.0, -0.0, 0.0, 0.0, -0.0, 1e-30, -1e-30, 2.0, 2.0, 7.25, -1e30, 1e30, float('inf'), float('-inf')])
    return pool[torch.randint(0, pool.numel(), (K, M), generator=g)].contiguous()       # negatives, both zeros, duplicates


def _check_sort(pg, K, M):
    for kind in ('normal', 'equal', 'descending', 'mixed'):
        x = _sort_rows(kind, K, M, M % 9973 + len(kind))
        got = pg.ops.swd_sort_rows_(x.clone().cuda()).cpu()
        assert torch.equal(got, x.sort(dim=1)[0]), (kind, K, M)


@pytest.mark.parametrize('M', [1, 2, 127, 1000, 4096])
def test_swd_sort_rows_small(pg, M):
    _check_sort(pg, 3, M)


def _switch_sizes():
    import pggan_amd as pg
    row, run, tile = pg.ops.SWD_SORT_LDS_ROW, pg.ops.SWD_SORT_MERGE_RUN, pg.ops.SWD_SORT_MERGE_TILE
    sizes = {row - 1, row, row + 1,                   # one workgroup in LDS | runs + merge
             run - 1, run + 1,                        # one run | a second, one-element run
             2 * run - 1, 2 * run, 2 * run + 1,       # one merge pass (the run sort lands in the scratch) | two (a third run without a partner)
             run + tile - 1, run + tile + 1,          # a merge tile that ends with the row | a last tile of one element
             3 * run + 5,                             # four runs, the last short: two passes, the run sort lands in buf
             4 * run + 1}                             # three passes (the run sort lands in the scratch), the fifth run rides along twice
    return sorted(sizes)


@pytest.mark.parametrize('M', _switch_sizes())
def test_swd_sort_rows_at_every_switch(pg, M):
    _check_sort(pg, 3, M)


def test_swd_sort_rows_long(pg):
    _check_sort(pg, 2, 2 ** 20 + 17)


def test_swd_sort_rows_argument_errors(pg):
    with pytest.raises(ValueError):
        pg.ops.swd_sort_rows_(torch.zeros(4).cuda())
    with pytest.raises(ValueError):
        pg.ops.swd_sort_rows_(torch.zeros(2, 0).cuda())
    big = torch.zeros(1, pg.ops.SWD_SORT_LDS_ROW + 1).cuda()
    with pytest.raises(ValueError):
        pg.ops.swd_sort_rows_(big, tmp=big)


# ------------------------------------------------------------------------------------------------- L1
@pytest.mark.parametrize('n', [1, 1000, 2 ** 20 + 3])
def test_swd_l1(pg, n):
    g = _gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    got = pg.ops.swd_l1(a.cuda(), b.cuda())
    assert got.dim() == 0 and got.is_cuda
    ref = float((a - b).double().abs().mean())          # (the fp32 difference is the kernel's input to the fp64 sum)
    ref64 = float((a.double() - b.double()).abs().mean())
    rel = abs(float(got) - ref64) / ref64
    print('swd_l1 n=%d: %.9g vs fp64 %.9g (rel %.3e; fp64 sum of fp32 differences %.9g)' % (n, float(got), ref64, rel, ref))
    assert rel <= 1e-6


# ------------------------------------------------------------------------------------------------- end to end
def _smooth(g, n=16):
    """8x8 Gaussian noise repeated x4 in both directions, plus 0.3 * noise"""
    low = torch.randn(n, 3, 8, 8, generator=g)
    return (low.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3) + 0.3 * torch.randn(n, 3, 32, 32, generator=g)).contiguous()


@pytest.fixture(scope='module')
def e2e_sets():
    g = _gen(11)
    return {'A': _smooth(g), 'B': _smooth(g), 'noise': torch.randn(16, 3, 32, 32, generator=g)}


def _run_metric(metric, real, fake, minibatch=5):
    metric.reset()
    for s in range(0, real.shape[0], minibatch):
        metric.feed_real(real[s:s + minibatch].contiguous().cuda())
        metric.feed_fake(fake[s:s + minibatch].contiguous().cuda())
    return metric.result()


@pytest.fixture(scope='module')
def e2e_metric(pg):
    return pg.metrics.SlicedWasserstein(32, 16, patches_per_image=32, dir_repeats=4, dirs_per_repeat=64, seed=1)


@pytest.mark.parametrize('pair', [('A', 'B'), ('A', 'noise'), ('A', 'A')])
def test_metric_end_to_end(pg, e2e_metric, e2e_sets, pair):
    m = e2e_metric
    assert m.levels == [32, 16] and tuple(m.directions.shape) == (4, 147, 64)
    assert float((m.directions.double().pow(2).sum(dim=1) - 1).abs().max()) < 1e-6
    for c, s in zip(m.centres, m.levels):
        assert tuple(c.shape) == (16 * 32, 2) and c.dtype == torch.int32 and int(c.min()) >= 3 and int(c.max()) <= s - 4
    real, fake = e2e_sets[pair[0]], e2e_sets[pair[1]]
    got = _run_metric(m, real, fake)
    ref = swd_ref.swd(real.double(), fake.double(), m.centres, m.directions.double(), 32)
    assert got['levels'] == [32, 16]
    for lv, a, b in zip(got['levels'], got['swd'], ref['swd']):
        print('SWD %s/%s level %d: device %.6f  fp64 %.6f  |diff| %.3e' % (pair[0], pair[1], lv, a, b, abs(a - b)))
    for a, b in zip(got['swd'] + [got['mean']], ref['swd'] + [ref['mean']]):
        assert abs(a - b) <= 1e-3
    if pair[0] == pair[1]:
        assert got['swd'] == [0.0, 0.0] and got['mean'] == 0.0
    else:
        assert min(got['swd']) > 10.0                                     # (different sets are whole units apart)


def test_metric_is_a_function_of_its_seed(pg, e2e_sets):
    kw = dict(patches_per_image=32, dir_repeats=4, dirs_per_repeat=64)
    a, b = e2e_sets['A'], e2e_sets['B']
    r1 = _run_metric(pg.metrics.SlicedWasserstein(32, 16, seed=1, **kw), a, b)
    r2 = _run_metric(pg.metrics.SlicedWasserstein(32, 16, seed=1, **kw), a, b, minibatch=16)
    r3 = _run_metric(pg.metrics.SlicedWasserstein(32, 16, seed=2, **kw), a, b)
    assert r1 == r2                                                       # bit for bit, whatever the split into minibatches
    assert r1['swd'] != r3['swd']


def test_metric_feed_errors(pg, e2e_sets):
    m = pg.metrics.SlicedWasserstein(32, 4, patches_per_image=4, dir_repeats=1, dirs_per_repeat=8)
    a = e2e_sets['A'].cuda()
    with pytest.raises(ValueError):
        m.feed_real(a[:5])                                                # more than num_images
    with pytest.raises(ValueError):
        m.feed_real(a[:2, :, :16, :16].contiguous())                      # another resolution
    m.feed_real(a[:4])
    with pytest.raises(RuntimeError):
        m.result()                                                        # no fake images yet


# ------------------------------------------------------------------------------------------------- the plugin
def test_swd_monitor_writes_the_metric_of_its_batches(pg):
    torch.manual_seed(3)
    G = pg.Generator((1, 3, 16, 16), latent_size=32, fmap_base=128, fmap_max=32)
    G.to('cuda')
    G.depth, G.alpha = 2, 1.0
    g = _gen(21)
    reals, fakes = [], []

    def real_batch_fn(n):
        reals.append(torch.randn(n, 3, 16, 16, generator=g).cuda())
        return reals[-1]

    def forward(z):
        fakes.append(G.forward(z).clone())                                # (a later pass may reuse the output buffer)
        return fakes[-1]

    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=0, G=types.SimpleNamespace(depth=2, forward=forward))
    mon = pg.SWDMonitor(real_batch_fn, lambda n: torch.randn(n, 32, generator=g), num_images=8, minibatch=3, swd_ticks=1,
                        patches_per_image=8)
    mon.register(trainer)
    mon.epoch(1)
    assert [r.shape[0] for r in reals] == [3, 3, 2] and [tuple(f.shape) for f in fakes] == [(3, 3, 16, 16), (3, 3, 16, 16), (2, 3, 16, 16)]
    direct = pg.metrics.SlicedWasserstein(16, 8, patches_per_image=8)
    direct.feed_real(torch.cat(reals))
    direct.feed_fake(torch.cat(fakes))
    res = direct.result()
    st = trainer.stats
    assert st['swd']['val'] == res['mean'] and st['swd_16']['val'] == res['swd'][0] and res['mean'] > 0
    assert st['swd']['log_name'] == 'swd' and st['swd']['log_epoch_fields'][0].format(**st['swd'])
    assert set(st) == {'swd', 'swd_16'}
