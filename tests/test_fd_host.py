"""The host tier of the Frechet distance over the random embedding: the binding of include/pggan_hip_embed.h, metrics.frechet_statistic
against closed forms, the host twin of metrics.RandomEmbedding / FrechetDistance (device='cpu') against tests/fd_ref.py and on synthetic
sets, plugins.FDMonitor on the twin with a stub trainer, and the argument errors.  Host tests: no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import fd_ref

import pggan_amd as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = pg.metrics


# ------------------------------------------------------------------------------------------------------------------ binding
def test_embed_header_is_derived_completely_and_the_product_tables_are_unchanged():
    _lib = pg._lib
    with open(os.path.join(ROOT, 'include', 'pggan_hip_embed.h')) as f:
        hdr = f.read()
    args, res, consts = _lib.parse_header(hdr)
    declared = set(re.findall(r'^int\s+(pg_\w+)\s*\(', hdr, flags=re.M))
    assert declared == set(args) == set(_lib.EMBED_SIGNATURES) == {'pg_emb_stem_u8_bf16', 'pg_emb_pool2_bf16', 'pg_emb_gap_f32',
                                                                   'pg_fd_moments_f64'}
    P, I, L = _lib.P, _lib.I, _lib.L
    assert _lib.EMBED_SIGNATURES == {'pg_emb_stem_u8_bf16': [P, P, L, I, I, I, P], 'pg_emb_pool2_bf16': [P, P, L, I, I, I, P],
                                     'pg_emb_gap_f32': [P, P, L, I, I, I, P], 'pg_fd_moments_f64': [P, L, I, P, P, P, L, P]}
    assert all(r is I for r in res.values())
    assert consts == _lib.EMBED_CONSTANTS == {'PG_EMB_STEM_CH': 8, 'PG_EMB_MAX_C': 4, 'PG_FD_SLICE': 256, 'PG_FD_TILE': 64,
                                              'PG_FD_MIN_F': 16, 'PG_FD_MAX_F': 512}
    assert (pg.ops.EMB_STEM_CH, pg.ops.EMB_MAX_C, pg.ops.FD_SLICE, pg.ops.FD_TILE) == (8, 4, 256, 64)
    # additive: the product boundary is what it was, and no name is declared twice
    assert len(_lib.SIGNATURES) == 96 and _lib.ABI_VERSION == 27
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'EMBED_SIGNATURES']
    assert len(others) >= 14 and not any(set(_lib.EMBED_SIGNATURES) & set(t) for t in others)
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('CONSTANTS') and n != 'EMBED_CONSTANTS']
    assert not any(set(_lib.EMBED_CONSTANTS) & set(t) for t in others)


def test_library_exports_the_embed_symbols():
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    for name in pg._lib.EMBED_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.pg_abi_version() == pg._lib.ABI_VERSION


def test_scratch_size():
    assert pg.ops.fd_moments_scratch(2, 16) == 16 + 4096
    assert pg.ops.fd_moments_scratch(513, 128) == 3 * (128 + 3 * 4096)
    assert pg.ops.fd_moments_scratch(256, 512) == 512 + 36 * 4096


# ---------------------------------------------------------------------------------------------------------------- the statistic
def _gaussian_moments(F, rows, seed, shift=0.0):
    x = np.random.RandomState(seed).randn(rows, F) * np.linspace(0.2, 3.0, F) + shift
    return fd_ref.moments(x)


def test_statistic_equal_moments():
    mu, cov = _gaussian_moments(128, 1024, 1)
    res = M.frechet_statistic(mu, cov, mu, cov)
    print('equal moments: fd = %.3e, bound %.3e' % (res['fd'], 1e-9 * 2 * np.trace(cov)))
    assert res['mean_term'] == 0.0 and res['fd'] == res['cov_term'] and abs(res['fd']) <= 1e-9 * 2 * np.trace(cov)


def test_statistic_diagonal_covariances():
    rs = np.random.RandomState(2)
    a, b = rs.rand(64) * 4 + 0.01, rs.rand(64) * 4 + 0.01
    mu1, mu2 = rs.randn(64), rs.randn(64)
    want = ((mu1 - mu2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    res = M.frechet_statistic(mu1, np.diag(a), mu2, np.diag(b))
    assert abs(res['fd'] - want) <= 1e-12 * want and abs(res['mean_term'] - ((mu1 - mu2) ** 2).sum()) <= 1e-12 * want
    assert res['fd'] == res['mean_term'] + res['cov_term']


def test_statistic_rank_deficient_is_finite_and_agrees_with_the_other_route():
    mu1, cov1 = _gaussian_moments(128, 40, 3)                             # 40 rows for 128 features: rank 39
    mu2, cov2 = _gaussian_moments(128, 1024, 4, shift=0.1)
    assert np.linalg.matrix_rank(cov1) == 39
    res = M.frechet_statistic(mu1, cov1, mu2, cov2)
    assert np.isfinite(res['fd']) and res['fd'] > 0
    scale = np.trace(cov1) + np.trace(cov2)
    other = fd_ref.frechet(mu1, cov1, mu2, cov2)
    print('rank deficient: fd = %.12g, by the eigenvalues of cov1 cov2 %.12g' % (res['fd'], other))
    # The 89 zero eigenvalues of the product come out as +-2^-52 |cov1| |cov2| in either route, and the statistic takes their square
    # roots, doubled: 2 x 89 x sqrt(2^-52 |cov1| |cov2|) per route is what the two may differ by, not 1e-9 of the traces.
    norms = np.linalg.eigvalsh(cov1)[-1] * np.linalg.eigvalsh(cov2)[-1]
    assert abs(res['fd'] - other) <= 2 * 2 * 89 * np.sqrt(2.0 ** -52 * norms)
    full = M.frechet_statistic(*(_gaussian_moments(128, 1024, 5) + _gaussian_moments(128, 1024, 6, shift=0.5)))
    assert abs(full['fd'] - fd_ref.frechet(*(_gaussian_moments(128, 1024, 5) + _gaussian_moments(128, 1024, 6, shift=0.5)))) <= 1e-9 * scale
    try:
        from scipy.linalg import sqrtm
    except ImportError:
        return
    second = ((mu1 - mu2) ** 2).sum() + scale - 2 * np.trace(sqrtm(cov1.dot(cov2))).real
    print('scipy.linalg.sqrtm: %.12g' % second)                          # (a second opinion only: sqrtm of a singular product is loose)
    assert abs(res['fd'] - second) <= 1e-5 * scale


def test_statistic_is_not_clamped_and_checks_shapes():
    mu, cov = _gaussian_moments(16, 64, 7)
    values = [M.frechet_statistic(mu, cov * s, mu, cov * s)['fd'] for s in (1.0, 3.0, 7.0, 0.37, 11.0, 0.013)]
    assert all(abs(v) <= 1e-9 * 2 * 11 * np.trace(cov) for v in values)
    with pytest.raises(ValueError):
        M.frechet_statistic(mu, cov, mu[:8], cov)
    with pytest.raises(ValueError):
        M.frechet_statistic(mu, cov[:8], mu, cov)


# ---------------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize('C,r', [(1, 8), (3, 16)])
def test_host_embedding_against_the_reference(C, r):
    x = fd_ref.box_images(5, C, r, 1, seed=10 * C + r)
    x[0, 0, 0, :4] = [0, 127, 128, 255]
    emb = M.RandomEmbedding(C, seed=3, device='cpu')
    stages = dict(emb.trace(torch.from_numpy(x)))
    nhwc_bits = lambda t: fd_ref.rne_bits(t.float().permute(0, 2, 3, 1).contiguous().numpy())
    assert np.array_equal(nhwc_bits(stages['stem']), fd_ref.stem(x)[..., :C])                      # the three ends: ==
    H = r
    while H > 4:
        assert np.array_equal(nhwc_bits(stages['pool%d' % H]), fd_ref.pool2(nhwc_bits(stages['conv%d' % H])))
        H //= 2
    assert np.array_equal(stages['gap'].numpy(), fd_ref.gap(nhwc_bits(stages['conv4'])))
    for H, cin, cout in fd_ref.layers(r):                                                          # the weights: the stated draw
        assert emb.layers(r) == fd_ref.layers(r) and torch.equal(emb.weights(H, cin).double(), fd_ref.weights(3, H, cin))
        assert tuple(emb.weights(H, cin).shape) == (3, 3, cout, cin) and emb.weights(H, cin).dtype == torch.bfloat16
    # The chain: both are fp64 convolutions of the same bf16 operands, rounded once per layer.  They may differ where a value lies within
    # an fp64 rounding error of a bf16 tie; one flipped activation moves by one bf16 ulp, at most 2^-6 below |v| = 4 (PixelNorm bounds
    # |v| by sqrt(128) < 16, typical values are below 4), and the features are means of 16 such activations.
    got, want = emb(torch.from_numpy(x)).numpy(), fd_ref.embed(x, seed=3)
    assert got.dtype == np.float32 and got.shape == (5, 128)
    diff = np.abs(got.astype(np.float64) - want)
    print('host twin against the reference chain C %d r %d: %d of %d features differ, largest %.3e' % (C, r, (diff > 0).sum(), diff.size, diff.max()))
    assert diff.max() <= 2.0 ** -6 and (diff > 0).mean() <= 0.01
    assert np.array_equal(M.RandomEmbedding(C, seed=3, chunk=1, device='cpu')(torch.from_numpy(x)).numpy(), got)
    assert not np.array_equal(M.RandomEmbedding(C, seed=4, device='cpu')(torch.from_numpy(x)).numpy(), got)


def test_host_embedding_reduces_above_max_resolution():
    x = fd_ref.box_images(3, 2, 16, 1, seed=5)
    low = pg.dataset.level_host(x, 1)
    a = M.RandomEmbedding(2, max_resolution=8, device='cpu')(torch.from_numpy(x))
    b = M.RandomEmbedding(2, max_resolution=8, device='cpu')(torch.from_numpy(np.ascontiguousarray(low)))
    assert torch.equal(a, b) and not torch.equal(a, M.RandomEmbedding(2, device='cpu')(torch.from_numpy(x)))


@pytest.fixture(scope='module')
def sets():
    """The synthetic one-channel sets of the design check at r = 16, 256 images each: noise box-filtered twice (two draws) and unfiltered."""
    return {'real': fd_ref.box_images(256, 1, 16, 2, seed=1), 'fresh': fd_ref.box_images(256, 1, 16, 2, seed=2),
            'noise': fd_ref.box_images(256, 1, 16, 0, seed=3)}


def test_host_metric_orders_the_synthetic_sets(sets):
    m = M.FrechetDistance(torch.from_numpy(sets['real']), device='cpu').fit()
    assert m.resolution == 16 and m.shape == (1, 16, 16) and tuple(m.mean.shape) == (128,) and tuple(m.cov.shape) == (128, 128)
    assert m.mean.dtype == m.cov.dtype == torch.float64 and torch.equal(m.cov, m.cov.t())
    assert sorted(m.indices.tolist()) == list(range(256))
    out = {}
    for name in ('real', 'fresh', 'noise'):
        m.reset()
        for s in range(0, 256, 100):
            m.feed_u8(torch.from_numpy(sets[name][s:s + 100]))
        out[name] = m.result()
        assert set(out[name]) == {'fd', 'mean_term', 'cov_term', 'num_real', 'num_fake'}
        assert (out[name]['num_real'], out[name]['num_fake']) == (256, 256)
        print('host twin, real against %-5s: fd = %.6g (mean term %.6g, cov term %.6g)'
              % (name, out[name]['fd'], out[name]['mean_term'], out[name]['cov_term']))
    trace2 = 2 * float(torch.trace(m.cov))
    assert abs(out['real']['fd']) <= 1e-9 * trace2                                  # a set against itself: the equal-moments bound
    assert 0 < out['fresh']['fd'] < out['noise']['fd']
    with pytest.raises(RuntimeError):
        m.feed_u8(torch.from_numpy(sets['real'][:2]))                               # result() was taken
    m.reset()
    m.feed(torch.from_numpy(sets['noise'].astype(np.float32) / 127.5 - 1))          # fp32 samples quantise to the same levels
    assert m.result() == out['noise']


def test_num_real_takes_a_seeded_subset(sets):
    m = M.FrechetDistance(torch.from_numpy(sets['real']), num_real=100, seed=5, device='cpu').fit()
    idx = m.indices.tolist()
    assert idx == torch.randperm(256, generator=torch.Generator().manual_seed(5))[:100].tolist()
    feats = M.RandomEmbedding(1, seed=5, device='cpu')(torch.from_numpy(sets['real'][idx]))
    mean, cov = M._moments_host(feats.numpy())
    assert np.array_equal(m.mean.numpy(), mean) and np.array_equal(m.cov.numpy(), cov)
    want_mean, want_cov = fd_ref.moments(feats.numpy())
    assert np.allclose(mean, want_mean, rtol=0, atol=1e-14) and np.allclose(cov, want_cov, rtol=0, atol=1e-14)
    m.feed_u8(torch.from_numpy(sets['fresh'][:64]))                                 # fewer fakes than features: finite
    res = m.result()
    assert np.isfinite(res['fd']) and (res['num_real'], res['num_fake']) == (100, 64)
    shared = M.FrechetDistance(torch.from_numpy(sets['real']), num_real=100, seed=5, device='cpu', embedding=m.embedding).fit()
    assert shared.embedding is m.embedding and torch.equal(shared.cov, m.cov)


# --------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    x = torch.from_numpy(fd_ref.box_images(8, 1, 8, 1, seed=14))
    for kw in (dict(channels=0), dict(channels=5), dict(channels=True), dict(channels=1, max_resolution=3), dict(channels=1, max_resolution=48),
               dict(channels=1, max_resolution=1024), dict(channels=1, chunk=0), dict(channels=1, seed=1.5)):
        with pytest.raises(ValueError):
            M.RandomEmbedding(device='cpu', **kw)
    emb = M.RandomEmbedding(1, device='cpu')
    for bad in (x.float(), x[:, :, :, :4], x.repeat(1, 2, 1, 1), x[:0], torch.zeros((2, 1, 2, 2), dtype=torch.uint8),
                torch.zeros((2, 1, 12, 12), dtype=torch.uint8), 'x'):
        with pytest.raises(ValueError):
            emb(bad)
    for kw in (dict(num_real=1), dict(num_real=2.5), dict(max_resolution=3), dict(max_resolution=1024), dict(drange=(1, 1)), dict(seed='a'),
               dict(embedding='x')):
        with pytest.raises((ValueError, TypeError)):
            M.FrechetDistance(x, device='cpu', **kw)
    with pytest.raises(ValueError):
        M.FrechetDistance(x.float(), device='cpu')
    with pytest.raises(ValueError):
        M.FrechetDistance(x, num_real=9, device='cpu').fit()                         # more than there are
    with pytest.raises(ValueError):
        M.FrechetDistance(x, device='cpu', embedding=M.RandomEmbedding(3, device='cpu')).fit()      # another channel count
    m = M.FrechetDistance(x, device='cpu')
    with pytest.raises(RuntimeError):
        m.feed_u8(x)                                                                 # fit() first
    with pytest.raises(RuntimeError):
        m.result()
    m.fit()
    with pytest.raises(ValueError):
        m.feed_u8(torch.zeros((2, 1, 16, 16), dtype=torch.uint8))                    # another shape
    with pytest.raises(ValueError):
        m.feed_u8(x.float())
    with pytest.raises(ValueError):
        m.feed(x)
    m.feed_u8(x[:1])
    with pytest.raises(RuntimeError):
        m.result()                                                                   # one fake
    for call in (lambda: pg.ops.emb_stem_u8_bf16(x), lambda: pg.ops.emb_pool2_bf16(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16)),
                 lambda: pg.ops.emb_gap_f32(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16)), lambda: pg.ops.fd_moments_f64(torch.zeros(4, 16))):
        with pytest.raises(ValueError):
            call()                                                                   # host tensors: the wrappers take device tensors only
    ds = types.SimpleNamespace()
    with pytest.raises(ValueError):
        pg.FDMonitor(ds, None, num_samples=1)
    with pytest.raises(ValueError):
        pg.FDMonitor(ds, None, minibatch=0)
    with pytest.raises(ValueError):
        pg.FDMonitor(ds, None, precision='fp8')


# ------------------------------------------------------------------------------------------------------------------ monitor
class _Latents(object):
    """What ``sample_fn`` returns on a host without a device: ``.cuda()`` hands the tensor on."""

    def __init__(self, z):
        self.z = z

    def cuda(self):
        return self.z


class _StubG(object):
    """'Generates' training images of the data set's current stage, picked by the latent's first column, plus a constant."""

    def __init__(self, ds, shift):
        self.ds, self.shift, self.calls = ds, shift, 0

    def forward(self, z):
        self.calls += 1
        level = self.ds.level_stack().float()
        idx = (z[:, 0].abs() * 1000).long() % level.shape[0]
        return ((level[idx] + self.shift).clamp(0, 255) / 127.5 - 1).contiguous()


def test_monitor_on_the_twin_refits_on_a_stage_change_and_respects_smoothed():
    stack = fd_ref.box_images(60, 1, 16, 2, seed=8)
    ds = pg.DeviceImageDataset(stack, model_initial_depth=1, device='cpu')      # 8x8
    G, Gs = _StubG(ds, 0.0), _StubG(ds, 40.0)
    trainer = types.SimpleNamespace(stats={}, parallel=None, cur_nimg=0, G=G, g_ema=types.SimpleNamespace(network=lambda: Gs))
    g = torch.Generator().manual_seed(2)
    drawn, latents = [], []

    def sample_fn(n):
        drawn.append(n)
        latents.append(torch.randn(n, 4, generator=g))
        return _Latents(latents[-1])

    mon = pg.FDMonitor(ds, sample_fn, num_samples=40, minibatch=16, fd_ticks=1, device='cpu')
    assert mon.trigger_interval == [(1, 'epoch'), (1, 'end')]
    mon.register(trainer)
    mon.epoch(1)
    st = trainer.stats
    assert set(st) == {'fd'} and drawn == [16, 16, 8] and (G.calls, Gs.calls) == (0, 3)
    metric = mon._metric_obj
    assert metric.resolution == 8 and tuple(metric.mean.shape) == (128,)
    res = metric.result()
    assert st['fd']['val'] == res['fd'] and np.isfinite(res['fd']) and res['fd'] > 0 and (res['num_real'], res['num_fake']) == (60, 40)
    fakes = M._quantise_host(torch.cat([_StubG(ds, 40.0).forward(z) for z in latents]).numpy(), (-1, 1))
    emb = M.RandomEmbedding(1, device='cpu')
    want = M.frechet_statistic(*(M._moments_host(emb(ds.level_stack()[metric.indices]).numpy())
                                 + M._moments_host(emb(torch.from_numpy(fakes)).numpy())))
    assert res['fd'] == want['fd']
    first = metric.cov.clone()
    mon.epoch(2)                                                                 # the same stage: no refit
    assert mon._metric_obj is metric and torch.equal(metric.cov, first)
    ds.model_depth = 2                                                           # 16x16
    mon.end(3)
    assert metric.resolution == 16 and metric.shape == (1, 16, 16) and not torch.equal(metric.cov, first)
    raw = pg.FDMonitor(ds, sample_fn, num_samples=8, minibatch=8, smoothed=False, max_resolution=8, num_real=30, device='cpu')
    raw.register(trainer)
    raw.epoch(1)
    assert G.calls == 1 and raw._metric_obj.embedding.max_resolution == 8 and raw._metric_obj.indices.numel() == 30
    with pytest.raises(ValueError):
        pg.FDMonitor(ds, sample_fn, smoothed=True, device='cpu').register(types.SimpleNamespace(g_ema=None))
    other = types.SimpleNamespace(stats={}, parallel=types.SimpleNamespace(rank=1), G=G, g_ema=None)
    raw.register(other)
    raw.epoch(1)
    assert other.stats == {}                                                     # rank 0 evaluates
    assert pg.FDMonitor(ds, sample_fn).precision == 'fp32' and pg.FDMonitor(ds, sample_fn, precision='bf16').precision == 'bf16'
