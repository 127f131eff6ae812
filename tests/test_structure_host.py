"""The two single statements the consumers share: the post-processor hand-over (``utils.run_postprocessors``) and the generator's stage
structure (``Generator.stage_convs`` / ``rgb_heads``).  Host only: stubs and object identities, no device."""
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
