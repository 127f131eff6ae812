"""The single statements the consumers share: the post-processor hand-over (``utils.run_postprocessors``), the generator's stage
structure (``Generator.stage_convs`` / ``rgb_heads``), and the bases of the uint8-space metrics and of their monitors (one
quantisation, one mirrored merge, one fitted feed, one batch loop).  Host only: stubs and object identities, no device."""
import pytest

import pggan_amd as pg


class _Batch(object):
    """Stands in for a device tensor: counts its host copies."""

    def __init__(self):
        self.copies = []

    def cpu(self):
        return self

    def numpy(self):
        self.copies.append(object())
        return self.copies[-1]


class _Proc(object):
    def __init__(self, device_tensors):
        if device_tensors:
            self.accepts_device_tensors = True
        self.got = []

    def __call__(self, batch, description):
        self.got.append((batch, description))


def test_run_postprocessors_hands_over_the_tensor_or_one_lazy_host_copy():
    batch = _Batch()
    host_a, dev, host_b = _Proc(False), _Proc(True), _Proc(False)
    assert pg.utils.run_postprocessors(batch, 'tick_7', [dev]) is None and batch.copies == []       # nobody asked for a host array yet
    pg.utils.run_postprocessors(batch, 'tick_7', [dev, host_a, host_b])
    assert [len(p.got) for p in (dev, host_a, host_b)] == [2, 1, 1]
    assert all(b is batch and d == 'tick_7' for b, d in dev.got)                                    # the tensor itself
    assert len(batch.copies) == 1                                                                   # one copy ...
    assert host_a.got == [(batch.copies[0], 'tick_7')] and host_b.got[0][0] is host_a.got[0][0]     # ... shared by both host stubs
    # no copy when every post-processor takes device tensors, and none without post-processors
    other = _Batch()
    pg.utils.run_postprocessors(other, 3, [_Proc(True), _Proc(True)])
    pg.utils.run_postprocessors(other, 3, [])
    assert other.copies == []
    # the copy is made when the first host-taking post-processor is reached, not before
    late, seen = _Batch(), []

    def watch(batch, description):
        seen.append(len(batch.copies))
    watch.accepts_device_tensors = True
    pg.utils.run_postprocessors(late, 3, [watch, _Proc(False), watch])
    assert seen == [0, 1] and len(late.copies) == 1


@pytest.fixture(scope='module')
def G():
    """A 32x32 generator: block0 and three blocks, so depth 0 .. 3.  (``fmap_base=64``: with 32 the last block would have 2 feature maps,
    and ``PGConv2d`` refuses channel counts that are no multiple of 4.)"""
    return pg.Generator((1, 3, 32, 32), fmap_base=64, fmap_max=16, latent_size=16)


@pytest.mark.parametrize('alpha', [1.0, 0.5])
@pytest.mark.parametrize('depth', [0, 1, 2, 3])
def test_stage_structure_is_the_parent_formulas(G, depth, alpha):
    assert len(G.blocks) == 3
    # stage_convs: block0's convs, then those of blocks[:depth], under their dotted names
    names = ['block0.c1', 'block0.c2'] + ['blocks.%d.%s' % (i, c) for i in range(depth) for c in ('c1', 'c2')]
    layers = [G.block0.c1, G.block0.c2] + [lay for i in range(depth) for lay in (G.blocks[i].c1, G.blocks[i].c2)]
    got = G.stage_convs(depth)
    assert [n for n, _ in got] == names
    assert len(got) == len(layers) and all(a is b for (_, a), b in zip(got, layers))
    modules = dict(G.named_modules())
    assert all(modules[n] is lay for n, lay in got)                                                 # the names are the modules' own
    # rgb_heads: the top block's toRGB and, while fading in, the one below
    head, previous = G.rgb_heads(depth, alpha)
    assert head is (G.blocks[depth - 1].toRGB if depth > 0 else G.block0.toRGB)
    if depth > 0 and alpha < 1.0:
        assert previous is (G.blocks[depth - 2].toRGB if depth > 1 else G.block0.toRGB)
    else:
        assert previous is None
    # the engine's walkers return what the hand-written formulas returned
    want = list(layers)
    want.append(G.blocks[depth - 1].toRGB if depth > 0 else G.block0.toRGB)
    if depth > 0 and alpha < 1.0:
        want.append(G.blocks[depth - 2].toRGB if depth > 1 else G.block0.toRGB)
    got = pg.engine.g_exchange_layers(G, depth, alpha)
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    G.depth, G.alpha = depth, alpha
    try:
        blocks = [G.block0] + list(G.blocks)[:depth]
        want = [m for b in blocks for m in (b.c1, b.c2)]
        got = pg.engine._live_conv_layers(G)
        assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    finally:
        G.depth, G.alpha = 0, 1.0
    # the samplers' and the projector's lists are slices of the same statement
    full = G.stage_convs(len(G.blocks))
    assert [n for n, _ in pg.sampling._conv3_layers(G)] == [n for n, _ in full[1:]]
    assert all(a is b for (_, a), (_, b) in zip(pg.sampling._conv3_layers(G), full[1:]))


# ----------------------------------------------------------------------------------- the uint8-space metrics and their monitors
def _planted_lists(K, k, shift, seed):
    """Two sorted lists of k keys per sample ([2 K, k] columns in key order, rows K .. 2 K - 1 the mirrored queries') with planted ties:
    equal sqdist with different index, equal (sqdist, index[, start]) in both lists, and for the shift form equal (sqdist, segment) with
    different start."""
    import numpy as np
    rng = np.random.RandomState(seed)
    cols = []
    for half in range(2):
        rows = []
        for i in range(K):
            keys = [(int(rng.randint(1, 4)), int(rng.randint(0, 4))) + ((int(rng.randint(0, 3)),) if shift else ()) for _ in range(k)]
            keys[0] = (0,) + keys[0][1:] if half == 0 else tuple(cols[0][i][0])   # the head of both lists: only ``mirrored`` differs
            if k > 1:
                keys[1] = (keys[0][0], keys[0][1] + 1) + keys[0][2:]           # equal sqdist, another index
            if shift and k > 2:
                keys[2] = keys[0][:2] + (keys[0][2] + 1,)                      # equal (sqdist, segment), another start
            rows.append(sorted(keys))
        cols.append(rows)
    both = np.asarray(cols[0] + cols[1], dtype=np.int64)                       # [2 K, k, keys]
    return [np.ascontiguousarray(both[:, :, j]) for j in range(both.shape[2])]


@pytest.mark.parametrize('shift', [False, True])
@pytest.mark.parametrize('k', [1, 2, 4])
def test_mirrored_merge_is_sorted_tuples(k, shift):
    import numpy as np
    K = 3
    columns = _planted_lists(K, k, shift, seed=10 * k + shift)
    merged = pg.metrics._LevelMetric._merge_mirrored(*columns)
    assert len(merged) == len(columns) + 1 and all(m.shape == (K, k) for m in merged) and merged[-1].dtype == np.bool_
    for i in range(K):
        want = sorted(tuple(int(c[i + K * m, j]) for c in columns) + (bool(m),) for m in (0, 1) for j in range(k))[:k]
        got = [tuple(int(m[i, j]) for m in merged[:-1]) + (bool(merged[-1][i, j]),) for j in range(k)]
        assert got == want
    ties = [tuple(int(c[0, 0]) for c in columns) == tuple(int(c[K, 0]) for c in columns)]
    assert all(ties) and not merged[-1][0, 0] and (k == 1 or merged[-1][0, 1])          # the planted equal key: unmirrored first


def test_levels_is_the_host_quantisation_and_its_flip():
    import numpy as np
    import torch
    x = torch.tensor([-1.2, -1.0, -0.99607843, 0.0, 0.00392157, 0.5, 1.0, 1.7, (2.5 / 127.5) - 1, (3.5 / 127.5) - 1], dtype=torch.float32)
    samples = x.repeat(10)[:96].reshape(2, 3, 4, 4).contiguous()               # the exact halves 2.5 and 3.5 among them
    stack = torch.zeros(4, 3, 4, 4, dtype=torch.uint8)
    for drange in ((-1, 1), (0, 1), (-2.5, 3.0)):
        nn = pg.metrics.NearestNeighbours(stack, drange=drange, device='cpu')
        want = pg.metrics._quantise_host(samples.numpy(), drange)
        got = nn._levels(samples)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
        both = nn._levels(samples, mirror=True)
        assert tuple(both.shape) == (4, 3, 4, 4) and np.array_equal(both[:2].numpy(), want)
        assert np.array_equal(both[2:].numpy(), want[..., ::-1]) and not np.array_equal(want, want[..., ::-1])


def test_pairs_share_one_statement():
    m, p = pg.metrics, pg.plugins
    # one quantisation, one merge, one sample check for the four metrics; one source check and one stack() for the three stack metrics
    for cls in (m.NearestNeighbours, m.ShiftNearestNeighbours, m.NDB, m.PrecisionRecall):
        for name in ('_levels', '_merge_mirrored', '_check_samples', '_check_range_in'):
            assert getattr(cls, name) is getattr(m._LevelMetric, name)
    for cls in (m.NearestNeighbours, m.NDB, m.PrecisionRecall):
        assert cls.stack is m._StackSource.stack and cls._stack_source is m._StackSource._stack_source
    for name in ('_fitted', 'feed', 'feed_u8'):
        assert getattr(m.NDB, name) is getattr(m.PrecisionRecall, name) is getattr(m._FittedFeed, name)
    assert m.NDB._take is not m.PrecisionRecall._take
    # the monitors: one evaluate per pair
    assert p.NNMonitor.evaluate is p.ShiftNNMonitor.evaluate is p._NeighbourSheet.evaluate
    assert p.NDBMonitor.evaluate is p.PRDMonitor.evaluate is p._FittedSamples.evaluate
    assert p.NDBMonitor._stage_resolution is p.PRDMonitor._stage_resolution is p._FittedSamples._stage_resolution
    assert (p.NNMonitor.metric, p.ShiftNNMonitor.metric) == ('NearestNeighbours', 'ShiftNearestNeighbours')
    assert pg.cluster._u8_images is pg.ops._u8_images


def test_feed_goes_through_levels_and_take():
    """Both fitted metrics quantise in ``_levels`` and hand the checked batch to their own ``_take``: a stub sees one call of each."""
    import torch
    stack = (torch.arange(8 * 16, dtype=torch.int64) * 37 % 256).to(torch.uint8).reshape(8, 1, 4, 4)
    for metric in (pg.metrics.NDB(stack, k=2, device='cpu'), pg.metrics.PrecisionRecall(stack, k=1, device='cpu')):
        metric.fit()
        calls = []
        levels, take = metric._levels, metric._take
        metric._levels = lambda samples, mirror=False: calls.append('levels') or levels(samples, mirror)
        metric._take = lambda images: calls.append(('take', images.dtype, tuple(images.shape))) or take(images)
        metric.feed(torch.zeros(3, 1, 4, 4))
        metric.feed_u8(stack[:2])
        assert calls == ['levels', ('take', torch.uint8, (3, 1, 4, 4)), ('take', torch.uint8, (2, 1, 4, 4))] and metric._fed == 5


@pytest.mark.parametrize('total,minibatch', [(1, 16), (16, 16), (17, 16), (33, 16)])
def test_batches_cover_the_total_in_order(total, minibatch):
    sizes = list(pg.plugins._batches(total, minibatch))
    assert sum(sizes) == total and all(0 < n <= minibatch for n in sizes)
    assert sizes == [minibatch] * (total // minibatch) + ([total % minibatch] if total % minibatch else [])
    # the four monitor loops are this generator: a stub metric sees exactly these sizes
    seen = []

    class Metric(object):
        resolution = 8

        def reset(self):
            pass

        def feed(self, batch):
            seen.append(batch)

        def result(self):
            return {}

    class Latents(int):
        def cuda(self):
            return self

    class Net(object):
        def forward(self, n):
            return int(n)

    class Dataset(object):
        shape = (1, 8, 8)

        def _stage(self):
            return None, 0, 0

    mon = pg.plugins._FittedSamples(1, Dataset(), Latents, total, minibatch, None, 'fp32')
    mon.make_metric, mon.write_stats, mon.generator = Metric, lambda res: None, Net
    mon.evaluate(0)
    assert seen == sizes
