"""GPU tier of the Frechet distance over the random embedding (csrc/embed.hip, metrics.RandomEmbedding / FrechetDistance,
plugins.FDMonitor) against tests/fd_ref.py.

The three ends of the embedding equal their numpy float32 twins with ==.  The moments are held to summation bounds that hold for ANY order:
the mean to (M + 1) 2^-53 sum|x| / M per column against exactly rounded sums, the covariance -- centred on the DEVICE's own mean, which
is what the kernel is specified to do -- to 2 (M + 4) 2^-53 sum_r |a_ri a_rj| / (M - 1) per element against math.fsum.  The 3x3 layers
are held to the conv contract of tests/test_sampling_gpu.py from the kernel's own inputs, under that criterion's own precondition.
Every comparison prints its measured maximum (as a ratio to the bound) before it asserts."""
import functools
import types

import numpy as np
import pytest
import torch

import fd_ref
import sampling_ref
from dataset_ref import make_stack
from test_sampling_gpu import held

import pggan_amd as pg

pytestmark = pytest.mark.gpu
M_ = pg.metrics
DEV = 'cuda'


def dev_bits(t):
    assert t.dtype == torch.bfloat16 and t.is_cuda
    return fd_ref.bits_of_tensor(t)


def bf16_dev(bits):
    return fd_ref.tensor_of_bits(bits).to(DEV).contiguous()


def some_bits(shape, seed):
    """bf16 activations like the embedding's: normal values up to a few units, some exact zeros and ties among them."""
    x = np.random.RandomState(seed).randn(*shape).astype(np.float32) * 1.5
    x.flat[::7] = 0.0
    return fd_ref.rne_bits(x)


# ------------------------------------------------------------------------------------------------------------------------- the ends
@pytest.mark.parametrize('r', [4, 8])
@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_stem_equals_its_twin(C, r):
    x = np.random.RandomState(10 * C + r).randint(0, 256, (3, C, r, r)).astype(np.uint8)
    x[:, :, 0, :4] = [0, 127, 128, 255]
    x.reshape(-1)[4:4 + min(256, x.size - 4)] = np.arange(min(256, x.size - 4))          # every level where the tensor has room
    y = pg.ops.emb_stem_u8_bf16(torch.from_numpy(x).to(DEV))
    assert tuple(y.shape) == (3, r, r, 8) and y.dtype == torch.bfloat16
    got, want = dev_bits(y), fd_ref.stem(x)
    assert np.array_equal(got, want) and not got[..., C:].any()
    assert {0, 127, 128, 255} <= set(x.reshape(-1).tolist())


@pytest.mark.parametrize('shape', [(2, 8, 8, 16), (1, 4, 4, 8)])
def test_pool_equals_its_twin(shape):
    bits = some_bits(shape, seed=shape[1])
    y = pg.ops.emb_pool2_bf16(bf16_dev(bits))
    assert tuple(y.shape) == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    assert np.array_equal(dev_bits(y), fd_ref.pool2(bits))


@pytest.mark.parametrize('shape', [(3, 4, 4, 128), (1, 4, 4, 8)])
def test_gap_equals_its_twin(shape):
    bits = some_bits(shape, seed=shape[3])
    f = pg.ops.emb_gap_f32(bf16_dev(bits))
    assert tuple(f.shape) == (shape[0], shape[3]) and f.dtype == torch.float32
    assert np.array_equal(f.cpu().numpy(), fd_ref.gap(bits))


def test_the_ends_refuse_what_they_do_not_take():
    with pytest.raises(ValueError):
        pg.ops.emb_stem_u8_bf16(torch.zeros((1, 5, 4, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        pg.ops.emb_pool2_bf16(torch.zeros((1, 3, 4, 8), dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError):
        pg.ops.emb_pool2_bf16(torch.zeros((1, 4, 4, 12), dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError):
        pg.ops.fd_moments_f64(torch.zeros((1, 16), device=DEV))
    with pytest.raises(ValueError):
        pg.ops.fd_moments_f64(torch.zeros((8, 24), device=DEV))
    with pytest.raises(ValueError):
        pg.ops.fd_moments_f64(torch.zeros((8, 528), device=DEV))
    x = torch.zeros((8, 16), device=DEV)
    out = torch.zeros(16 + 256 + 4096 + 16, dtype=torch.float64, device=DEV)
    stream = pg.ops._stream()
    rc = pg._lib.load().pg_fd_moments_f64(x.data_ptr(), 8, 16, out.data_ptr(), out[16:].data_ptr(), out[272:].data_ptr(), 4111, stream)
    assert rc == pg._lib.CONSTANTS['PG_E_ARG']                                  # the scratch is one value short: nothing is launched
    rc = pg._lib.load().pg_fd_moments_f64(x.data_ptr() + 4, 8, 16, out.data_ptr(), out[16:].data_ptr(), out[272:].data_ptr(), 4112, stream)
    assert rc == pg._lib.CONSTANTS['PG_E_ALIGN']


# ---------------------------------------------------------------------------------------------------------------------- the moments
def test_moments_of_small_integers_are_exact():
    """The accumulator map of the fp64 matrix instruction, checked with numbers that round nowhere: integer data whose column means are
    integers, so every centred value, product and sum is an integer and only the last division rounds.  One wrong row or column shows."""
    rs = np.random.RandomState(3)
    half = rs.randint(-30, 31, (6, 32))
    c = rs.randint(-5, 6, (1, 32))
    x = np.concatenate([half, 2 * c - half]).astype(np.float32)                 # column sums 12 c
    mean, cov = pg.ops.fd_moments_f64(torch.from_numpy(x).to(DEV))
    a = x.astype(np.int64) - c
    assert np.array_equal(mean.cpu().numpy(), c[0].astype(np.float64))
    assert np.array_equal(cov.cpu().numpy(), a.T.dot(a).astype(np.float64) / 11.0)
    assert len(set(a.T.dot(a)[np.triu_indices(32)].tolist())) > 400              # (of 528: the elements are told apart)


@functools.lru_cache(maxsize=None)
def moments_case(M, F, offset):
    rs = np.random.RandomState(1000 * F + M)
    x = (rs.randn(M, F) * np.linspace(0.1, 2.0, F) + rs.randn(1, F) + offset).astype(np.float32)
    return x


@pytest.mark.parametrize('M,F,offset', [(2, 16, 0.0), (5, 16, 0.0), (67, 48, 0.0), (300, 128, 0.0), (513, 128, 0.0), (300, 128, 1000.0)])
def test_moments_within_the_summation_bounds(M, F, offset):
    x = moments_case(M, F, offset)                                              # (shared, never modified)
    xd = torch.from_numpy(x).to(DEV)
    mean_d, cov_d = pg.ops.fd_moments_f64(xd)
    assert mean_d.dtype == cov_d.dtype == torch.float64 and tuple(mean_d.shape) == (F,) and tuple(cov_d.shape) == (F, F)
    mean, cov = mean_d.cpu().numpy(), cov_d.cpu().numpy()
    u = 2.0 ** -53
    mean_bound = (M + 1) * u * np.abs(x.astype(np.float64)).sum(axis=0) / M
    mean_err = np.abs(mean - fd_ref.mean_exact(x))
    print('moments (%d, %d) offset %g: mean largest error / bound = %.4f' % (M, F, offset, (mean_err / mean_bound).max()))
    want, mag = fd_ref.cov_exact(x, mean)                                       # centred on the device's own mean
    cov_bound = 2 * (M + 4) * u * mag / (M - 1)
    cov_err = np.abs(cov - want)
    print('moments (%d, %d) offset %g: cov largest error / bound = %.4f (largest error %.3e)'
          % (M, F, offset, (cov_err / cov_bound).max(), cov_err.max()))
    assert np.isfinite(mean).all() and (mean_err <= mean_bound).all()
    assert np.isfinite(cov).all() and (cov_err <= cov_bound).all()
    assert np.array_equal(cov, cov.T)
    mean_2, cov_2 = pg.ops.fd_moments_f64(xd)
    assert torch.equal(mean_2, mean_d) and torch.equal(cov_2, cov_d)            # two calls: the same bits
    if offset:
        # an uncentred form (sum x x^T - M mean mean^T) cancels 1e6-sized terms to a result of order 1: it would miss the bound by far
        x64 = x.astype(np.float64)
        naive = (x64.T.dot(x64) - M * np.outer(mean, mean)) / (M - 1)
        assert (np.abs(naive - want) > cov_bound).any()


# -------------------------------------------------------------------------------------------------------------------- the embedding
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('r', [8, 16])
def test_embedding_layer_by_layer(C, r):
    x = fd_ref.box_images(3, C, r, 1, seed=10 * C + r)
    xd = torch.from_numpy(x).to(DEV)
    emb = M_.RandomEmbedding(C, seed=3)
    stages = emb.trace(xd)
    names = [n for n, _ in stages]
    assert names[0] == 'stem' and names[-1] == 'gap' and names[-2] == 'conv4' and len(names) == 2 * len(fd_ref.layers(r)) + 1
    cur = dev_bits(stages[0][1])
    assert np.array_equal(cur, fd_ref.stem(x))
    for (name, t), (H, cin, cout) in zip([s for s in stages if s[0].startswith('conv')], fd_ref.layers(r)):
        assert name == 'conv%d' % H and tuple(t.shape) == (3, H, H, cout) and cur.shape == (3, H, H, cin)
        wb = fd_ref.weights(3, H, cin)
        assert torch.equal(emb.weights(H, cin).cpu().double(), wb)
        y_ref = fd_ref.layer(cur, wb, torch.float64, rounded=False)               # from the kernel's OWN input
        e32 = float((fd_ref.layer(cur, wb, torch.float32, rounded=False).double() - y_ref).abs().max())
        median_half_ulp = float(sampling_ref.half_ulp_bf16(y_ref[y_ref != 0]).median())
        print('C %d r %d %s: e32 = %.3e, median half-ulp = %.3e' % (C, r, name, e32, median_half_ulp))
        assert 3 * e32 < median_half_ulp / 100                                    # the condition of the criterion: the bf16 term decides
        held('C %d r %d %s' % (C, r, name), t, y_ref, sampling_ref.contract_bound(y_ref, e32))
        cur = dev_bits(t)
        if H > 4:
            pooled = dict(stages)['pool%d' % H]
            assert np.array_equal(dev_bits(pooled), fd_ref.pool2(cur))
            cur = dev_bits(pooled)
    feats = dict(stages)['gap']
    assert np.array_equal(feats.cpu().numpy(), fd_ref.gap(cur)) and tuple(feats.shape) == (3, 128)
    again = emb(xd)
    assert torch.equal(again, feats) and torch.equal(emb(xd), again)             # two calls: the same bits
    assert torch.equal(M_.RandomEmbedding(C, seed=3, chunk=1)(xd), feats) and torch.equal(M_.RandomEmbedding(C, seed=3, chunk=64)(xd), feats)
    host = M_.RandomEmbedding(C, seed=3, device='cpu')(torch.from_numpy(x))
    print('C %d r %d: device features against the host twin, largest difference %.3e' % (C, r, float((host - feats.cpu()).abs().max())))


def test_a_layer_has_the_same_weights_at_every_resolution():
    emb = M_.RandomEmbedding(1, seed=7)
    assert emb.layers(8)[1:] == emb.layers(16)[2:] == [(4, 128, 128)] and emb.layers(16)[1] == (8, 128, 128)
    x8, x16 = (torch.from_numpy(fd_ref.box_images(2, 1, r, 1, seed=r)).to(DEV) for r in (8, 16))
    emb(x8)
    w4 = emb.weights(4, 128)
    ptr, bits = w4.data_ptr(), dev_bits(w4).copy()
    emb(x16)
    assert emb.weights(4, 128).data_ptr() == ptr and np.array_equal(dev_bits(emb.weights(4, 128)), bits)    # uploaded once and kept
    assert np.array_equal(bits, fd_ref.bits_of_tensor(fd_ref.weights(7, 4, 128).to(torch.bfloat16)))
    other = M_.RandomEmbedding(1, seed=7)
    other(x16)                                                                    # another object, r = 16 first: the same draw
    assert np.array_equal(dev_bits(other.weights(4, 128)), bits)
    assert np.array_equal(dev_bits(other.weights(8, 128)), fd_ref.bits_of_tensor(fd_ref.weights(7, 8, 128).to(torch.bfloat16)))


# ----------------------------------------------------------------------------------------------------------------------- end to end
def test_device_metric_orders_the_synthetic_sets_as_the_host_twin_does():
    """r = 16, 1024 one-channel images per set.  No tolerance between the device and the twin is asserted (the twin is close, not
    equal): both values are printed; docs/experiments_fd.md records them."""
    n = 1024
    sets = {'real': fd_ref.box_images(n, 1, 16, 2, seed=1), 'fresh': fd_ref.box_images(n, 1, 16, 2, seed=2),
            'smoother': fd_ref.box_images(n, 1, 16, 3, seed=4), 'noise': fd_ref.box_images(n, 1, 16, 0, seed=3)}
    dev = M_.FrechetDistance(torch.from_numpy(sets['real']).to(DEV)).fit()
    twin = M_.FrechetDistance(torch.from_numpy(sets['real']), device='cpu').fit()
    assert dev.mean.is_cuda and dev.cov.dtype == torch.float64 and torch.equal(dev.cov, dev.cov.t())
    got, want = {}, {}
    for name, images in sets.items():
        dev.reset()
        twin.reset()
        for s in range(0, n, 400):
            dev.feed_u8(torch.from_numpy(images[s:s + 400]).to(DEV))
        twin.feed_u8(torch.from_numpy(images))
        got[name], want[name] = dev.result(), twin.result()
        print('real against %-8s: fd device %.9g, host twin %.9g, difference %.3e'
              % (name, got[name]['fd'], want[name]['fd'], got[name]['fd'] - want[name]['fd']))
        assert np.isfinite(got[name]['fd']) and (got[name]['num_real'], got[name]['num_fake']) == (n, n)
        assert got[name]['fd'] == got[name]['mean_term'] + got[name]['cov_term']
    order = lambda res: sorted(res, key=lambda k: res[k]['fd'])
    assert order(got) == order(want) == ['real', 'fresh', 'smoother', 'noise']
    assert abs(got['real']['fd']) <= 1e-9 * 2 * float(torch.trace(dev.cov))       # a set against itself (fed in another row order)
    dev.reset()
    dev.feed(torch.from_numpy(sets['noise'].astype(np.float32) / 127.5 - 1).to(DEV))
    assert dev.result() == got['noise']                                          # fp32 samples quantise to the same levels; the same bits


def test_monitor_on_a_tiny_network_through_a_stage_change(deterministic_forward):
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

    mon = pg.FDMonitor(ds, sample_fn, num_samples=40, minibatch=16, fd_ticks=1)
    mon.register(trainer)
    fits = []
    for depth, resolution in ((1, 8), (1, 8), (2, 16)):
        G.depth = ds.model_depth = depth
        del drawn[:]
        trainer.stats.clear()
        mon.epoch(1)
        st = trainer.stats
        assert set(st) == {'fd'} and [z.shape[0] for z in drawn] == [16, 16, 8]
        metric = mon._metric_obj
        assert metric.resolution == resolution and metric.shape == (3, resolution, resolution)
        fits.append(metric.cov)
        check = M_.FrechetDistance(ds).fit()
        assert torch.equal(check.mean, metric.mean) and torch.equal(check.cov, metric.cov)
        for z in drawn:
            check.feed(G.forward(z.cuda()))
        res = check.result()
        assert st['fd']['val'] == res['fd'] and np.isfinite(res['fd']) and res['fd'] > 0 and res['num_fake'] == 40
    assert fits[0] is fits[1] and fits[1] is not fits[2]                          # refitted once, at the stage change
