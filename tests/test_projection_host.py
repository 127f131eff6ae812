"""CPU tier of the latent projection (pggan-pytorch_amd/projection.py, include/pggan_hip_projection.h): the definition the GPU tests
are held to is pinned against autograd, the header parses into tables of its own and is bound by ``load()``, ``ops.pyramid_loss`` and
``Projector`` refuse every bad argument before a launch (nothing here has a device), and ``ProjectionMonitor`` follows the monitors'
conventions against a stub trainer."""
import inspect

import pytest
import torch

import projection_ref as ref

import pggan_amd as pg

ops = pg.ops


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize('N,C,r,weights', [(2, 1, 4, None), (2, 3, 8, None), (1, 2, 64, None), (2, 4, 32, [1.0, 0.0, 2.5]),
                                           (1, 1, 128, [0.5, 0.25, 0.0, 0.0, 3.0, 1.0])])
def test_closed_form_gradient_is_autograd_of_the_loss(N, C, r, weights):
    g = torch.Generator().manual_seed(r + C)
    img = torch.randn(N, C, r, r, generator=g, dtype=torch.float64).requires_grad_(True)
    tgt = torch.randn(N, C, r, r, generator=g, dtype=torch.float64)
    loss, grad = ref.pyramid_loss_ref(img.detach(), tgt, weights)
    auto_loss = ref.pyramid_loss_torch(img, tgt, weights)
    auto, = torch.autograd.grad(auto_loss.sum(), img)
    auto_loss = auto_loss.detach()
    assert float((loss - auto_loss).abs().max()) <= 1e-12 * float(auto_loss.abs().max())
    assert float((grad - auto).abs().max()) <= 1e-12 * float(auto.abs().max())
    lo, gb = ref.pyramid_bounds_ref(img.detach(), tgt, weights)
    assert bool((lo >= loss.abs() * (1 - 1e-12)).all()) and bool((gb >= grad.abs() * (1 - 1e-12)).all())


def test_levels_and_an_independent_spelling():
    assert [ref.levels(r) for r in (4, 8, 16, 64, 1024)] == [1, 2, 3, 5, 9]
    assert [ops.pyramid_levels(r) for r in (4, 8, 16, 64, 1024)] == [1, 2, 3, 5, 9]
    # r = 8, written out: level 0 is the pixels, level 1 the 4x4 grid of 2x2 means
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(1, 1, 8, 8, generator=g, dtype=torch.float64), torch.randn(1, 1, 8, 8, generator=g, dtype=torch.float64)
    e = a - b
    p1 = e.reshape(1, 1, 4, 2, 4, 2).mean(dim=(3, 5))
    want = (e ** 2).mean() + 3.0 * (p1 ** 2).mean()
    loss, grad = ref.pyramid_loss_ref(a, b, [1.0, 3.0])
    assert abs(float(loss[0]) - float(want)) <= 1e-14 * float(want)
    want_g = 2.0 / 64 * e + 3.0 * 2.0 / 16 / 4 * p1.repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert float((grad - want_g).abs().max()) <= 1e-15


# ------------------------------------------------------------------------------------------------ the header and the binding
def test_header_parses_into_its_own_tables_and_load_binds_them():
    sig, const = pg._lib.PROJECTION_SIGNATURES, pg._lib.PROJECTION_CONSTANTS
    assert set(sig) == {'pg_pyr_loss_grad'}
    P, I = pg._lib.P, pg._lib.I
    assert sig['pg_pyr_loss_grad'] == [P, P, P, I, P, P, P, pg._lib.ctypes.c_size_t, I, I, I, P]
    assert const['PG_PYR_TILE'] == 64 and const['PG_PYR_MAX_SIDE'] == 1024 and const['PG_PYR_MAX_C'] == 4
    assert const['PG_PYR_MAX_LEVELS'] == ref.levels(const['PG_PYR_MAX_SIDE']) and const['PG_PYR_SCRATCH_PER_TILE'] == 9
    others = (pg._lib.SIGNATURES, pg._lib.DEBUG_SIGNATURES, pg._lib.CLUSTER_SIGNATURES, pg._lib.GAN_SIGNATURES, pg._lib.PHASE_SIGNATURES,
              pg._lib.SAMPLING_SIGNATURES)
    assert all(not set(sig) & set(o) for o in others)
    assert not set(const) & set(pg._lib.CONSTANTS)
    assert 'PROJECTION_SIGNATURES' in inspect.getsource(pg._lib.load)            # the list load() binds
    lib = pg._lib.load()                                                       # (the library is built before the suite runs)
    assert lib.pg_pyr_loss_grad.argtypes == sig['pg_pyr_loss_grad']
    assert ops.pyramid_scratch_words(2, 3, 8) == 9 * 6 and ops.pyramid_scratch_words(1, 2, 128) == 9 * 2 * 4


# ------------------------------------------------------------------------------------------------ refusals before a launch
def test_pyramid_loss_refuses_host_tensors_and_bad_shapes():
    a = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match='img'):
        ops.pyramid_loss(a, a)
    with pytest.raises(ValueError, match='img'):
        ops.pyramid_loss([[0.0]], a)

    class Fake(torch.Tensor):
        """A tensor that claims to be on the device: the shape checks are reached without one."""
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)
    with pytest.raises(ValueError, match='target'):
        ops.pyramid_loss(fake(2, 3, 8, 8), fake(2, 3, 8, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match='equal shapes'):
        ops.pyramid_loss(fake(2, 3, 8, 8), fake(2, 3, 16, 16))
    with pytest.raises(ValueError, match='equal shapes'):
        ops.pyramid_loss(fake(3, 8, 8), fake(3, 8, 8))
    for shape in ((2, 5, 8, 8), (2, 3, 8, 4), (2, 3, 2, 2), (2, 3, 12, 12), (0, 3, 8, 8), (1, 1, 2048, 2048)):
        with pytest.raises(ValueError, match='power of two'):
            ops.pyramid_loss(fake(*shape), fake(*shape))
    x = fake(2, 3, 8, 8)
    for bad in ([], [1.0, 1.0, 1.0], [1.0, -0.5], [float('nan')], [float('inf')]):
        with pytest.raises(ValueError, match='weights'):
            ops.pyramid_loss(x, x, weights=bad)
    with pytest.raises(ValueError, match='scratch'):
        ops.pyramid_loss(x, x, scratch=torch.zeros(9 * 6 - 1, dtype=torch.float64))          # one word short
    with pytest.raises(ValueError, match='scratch'):
        ops.pyramid_loss(x, x, scratch=torch.zeros(9 * 6))                                   # not float64
    with pytest.raises(ValueError, match='img'):
        ops.pyramid_loss(fake(2, 3, 8, 16)[..., ::2], x)                                     # not contiguous


def _small_generator(**kw):
    return pg.Generator((1, 3, 8, 8), fmap_base=32, fmap_max=16, latent_size=16, **kw)


def test_projector_validates_its_arguments():
    G = _small_generator()
    with pytest.raises(ValueError, match='Generator'):
        pg.Projector(torch.nn.Linear(2, 2))
    for kw, what in ((dict(steps=0), 'steps'), (dict(steps=2.5), 'steps'), (dict(steps=True), 'steps'), (dict(lr=0.0), 'lr'),
                     (dict(lr=float('nan')), 'lr'), (dict(betas=(0.9,)), 'betas'), (dict(betas=(0.9, 1.0)), 'betas'), (dict(eps=0.0), 'eps'),
                     (dict(level_weights=[]), 'level_weights'), (dict(level_weights=[1.0, -1.0]), 'level_weights'),
                     (dict(level_weights=[1.0, 1.0, 1.0]), 'level_weights')):                # an 8x8 network has two levels
        with pytest.raises(ValueError, match=what):
            pg.Projector(G, **kw)
    with pytest.raises(ValueError, match='channels'):
        pg.Projector(pg.Generator((1, 5, 8, 8), fmap_base=32, fmap_max=16, latent_size=16))
    p = pg.Projector(G, steps=7, lr=0.05, betas=(0.5, 0.9), level_weights=[1.0, 0.5], seed=3)
    assert (p.steps, p.lr, p.betas, p.level_weights, p.seed) == (7, 0.05, (0.5, 0.9), [1.0, 0.5], 3)
    assert p.learning_rate(0) == 0.05 and abs(p.learning_rate(7)) < 1e-17 and abs(p.learning_rate(3.5) - 0.025) < 1e-17
    assert p.packed_weights() is None


def test_projector_has_no_cpu_path_and_refuses_before_a_launch():
    G = _small_generator()
    p = pg.Projector(G)
    with pytest.raises(RuntimeError, match='device'):
        p.project(torch.zeros(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match='device'):
        p.loss_and_grad(torch.zeros(2, 16), torch.zeros(2, 3, 4, 4))
    assert p.packed_weights() is None


def test_projector_sets_nothing_on_the_network_and_refers_to_it_weakly():
    import gc
    import weakref
    G = _small_generator()
    before = {id(m): dict(vars(m)) for m in G.modules()}
    rt_before = {k: getattr(G._rt, k, None) for k in G._rt.__slots__}
    p = pg.Projector(G)
    assert {id(m): dict(vars(m)) for m in G.modules()} == before
    assert {k: getattr(G._rt, k, None) for k in G._rt.__slots__} == rt_before
    assert p.network() is G
    w = weakref.ref(G)
    del G, before
    gc.collect()
    assert w() is None
    with pytest.raises(RuntimeError, match='gone'):
        p.network()


# ------------------------------------------------------------------------------------------------ the monitor
class _Trainer(object):
    parallel = None
    g_ema = None
    cur_nimg = 12000

    def __init__(self, G):
        self.G = G
        self.stats = {}


class _Result(object):
    def __init__(self, targets):
        self.images = targets + 1.0
        self.loss = torch.tensor([0.25, 0.75, 0.5][:targets.shape[0]])


class _StubProjector(object):
    seen = []

    def __init__(self, net, **kw):
        self.net, self.kw = net, kw

    def project(self, targets):
        _StubProjector.seen.append((self.net, self.kw, targets))
        return _Result(targets)


def test_monitor_refusals():
    fn = lambda n: torch.zeros(n, 3, 4, 4)
    with pytest.raises(ValueError, match='precision'):
        pg.ProjectionMonitor(fn, precision='fp16')
    with pytest.raises(ValueError, match='bf16'):
        pg.ProjectionMonitor(fn, precision='bf16')
    for kw in (dict(num_images=0), dict(num_images=2.5), dict(steps=0), dict(steps=True)):
        with pytest.raises(ValueError):
            pg.ProjectionMonitor(fn, **kw)
    with pytest.raises(ValueError, match='source'):
        pg.ProjectionMonitor(None)
    m = pg.ProjectionMonitor(fn, smoothed=True)
    with pytest.raises(ValueError, match='g_ema'):
        m.register(_Trainer(_small_generator()))
    pg.ProjectionMonitor(fn, smoothed=None).register(_Trainer(_small_generator()))           # falls back to G
    assert pg.ProjectionMonitor(fn).precision == 'fp32'


def test_monitor_tick_gating_stat_names_and_fixed_targets(monkeypatch):
    monkeypatch.setattr(pg.projection, 'Projector', _StubProjector)
    _StubProjector.seen = []
    calls = []

    def real_batch_fn(n):
        calls.append(n)
        return torch.full((n, 3, 4, 4), float(len(calls)))
    shown = []

    def proc(batch, description):
        shown.append((batch, description))
    proc.accepts_device_tensors = True                                                       # (gets the tensor, not a numpy copy)
    m = pg.ProjectionMonitor(real_batch_fn, num_images=3, steps=5, projection_ticks=7, postprocessors=[proc], lr=0.02)
    assert m.trigger_interval == [(7, 'epoch'), (1, 'end')]                                  # the trainer gates on this
    assert pg.ProjectionMonitor(real_batch_fn).trigger_interval == [(30, 'epoch'), (1, 'end')]
    G = _small_generator()
    tr = _Trainer(G)
    m.register(tr)
    assert tr.stats == {}
    m.epoch(7)
    m.epoch(14)
    m.end(15)
    assert calls == [3]                                                                      # drawn once, kept
    assert len(_StubProjector.seen) == 3 and all(s[0] is G and s[1] == dict(steps=5, lr=0.02) for s in _StubProjector.seen)
    assert all(s[2] is _StubProjector.seen[0][2] for s in _StubProjector.seen)               # the same targets at every tick
    assert set(tr.stats) == {'proj_loss', 'proj_loss_max'}
    assert tr.stats['proj_loss']['val'] == 0.5 and tr.stats['proj_loss_max']['val'] == 0.75
    assert tr.stats['proj_loss']['log_name'] == 'proj_loss' and tr.stats['proj_loss']['log_epoch_fields']
    batch, description = shown[0]
    assert description == 'proj_000012' and tuple(batch.shape) == (6, 3, 4, 4)
    assert torch.equal(batch[0::2], _StubProjector.seen[0][2]) and torch.equal(batch[1::2], _StubProjector.seen[0][2] + 1.0)
    # a new growth stage draws its own targets, once
    G.depth = 1
    with pytest.raises(ValueError, match='8x8'):
        m.epoch(21)                                                                          # (this stub source ignores the stage)

    class Rank1(object):
        rank = 1
    tr.parallel = Rank1()
    n = len(_StubProjector.seen)
    m.epoch(28)
    assert len(_StubProjector.seen) == n                                                     # rank 0 evaluates


def test_monitor_takes_the_tail_of_a_dataset(monkeypatch):
    monkeypatch.setattr(pg.projection, 'Projector', _StubProjector)
    _StubProjector.seen = []

    class Dataset(object):
        device = 'cpu'

        def __len__(self):
            return 10

        def items(self, idx, alpha=1.0):
            assert alpha == 1.0
            return idx.float().view(-1, 1, 1, 1).expand(-1, 3, 4, 4).contiguous()
    with pytest.raises(ValueError, match='11 targets'):
        pg.ProjectionMonitor(Dataset(), num_images=11)
    m = pg.ProjectionMonitor(Dataset(), num_images=3)
    tr = _Trainer(_small_generator())
    m.register(tr)
    m.epoch(1)
    m.epoch(2)
    a, b = _StubProjector.seen[0][2], _StubProjector.seen[1][2]
    assert a[:, 0, 0, 0].tolist() == [7.0, 8.0, 9.0] and torch.equal(a, b)


def test_exports():
    assert pg.Projector is pg.projection.Projector and pg.ProjectionMonitor is pg.plugins.ProjectionMonitor
    assert pg.project_samples is pg.utils.project_samples
    assert {'Projector', 'ProjectionMonitor', 'project_samples'} <= set(pg.__all__)
    sig = inspect.signature(pg.Projector.__init__).parameters
    assert [sig[k].default for k in ('steps', 'lr', 'betas', 'level_weights', 'seed')] == [200, 0.1, (0.9, 0.999), None, 0]
    assert list(inspect.signature(pg.utils.project_samples).parameters)[:4] == ['generator_path', 'targets', 'postprocessors', 'description']
