"""Host logic of the smoothed generator (ema.GeneratorEMA, Trainer(g_ema=...), the plugins' ``smoothed`` switch, saver and loader) on CPU
tensors, the kernels replaced by tests/emu_ops.py plus tests/emu_ema.py's statement of ``pg_ema_f32``.  The kernel itself and the stream
placement are checked on the device (tests/test_ema_gpu.py)."""
import importlib
import types

import numpy as np
import pytest
import torch

import emu_ema
import emu_ops

import pggan_amd as pg

SHAPE = (1, 3, 16, 16)
KW = dict(fmap_base=128, fmap_max=32)
LATENT = 32


@pytest.fixture()
def emu(monkeypatch):
    monkeypatch.setattr(emu_ops, 'ema', emu_ema.ema, raising=False)
    for modname in ('engine', 'optim', 'ema'):
        mod = importlib.import_module('pggan-pytorch_amd.' + modname)
        monkeypatch.setattr(mod, 'ops', emu_ops)
    monkeypatch.setattr(pg.engine, '_check_dev', lambda t, what: t.contiguous())
    monkeypatch.setattr(pg.trainer, '_to_device', lambda t: t)
    yield


class _Run(object):
    """A narrow 16x16 pair under Trainer on CPU tensors, minibatch 4, growth stage set by hand."""

    def __init__(self, seed=11, depth=1, trainer_kw=None, ema_kw=None, G=None, D=None):
        torch.manual_seed(seed)
        self.G = G if G is not None else pg.Generator(SHAPE, latent_size=LATENT, **KW)
        self.D = D if D is not None else pg.Discriminator(SHAPE, **KW)
        self.rs = np.random.RandomState(seed)
        self.ema = None if ema_kw is None else pg.GeneratorEMA(self.G, **ema_kw)
        opt_g = pg.FusedAdam(self.G.parameters(), 0.001, betas=(0.0, 0.99))
        opt_d = pg.FusedAdam(self.D.parameters(), 0.001, betas=(0.0, 0.99))
        kw = dict(trainer_kw or {})
        if self.ema is not None:
            kw['g_ema'] = self.ema
        self.tr = pg.Trainer(self.D, self.G, self._d_loss, pg.wgan_gp_G_loss, opt_d, opt_g, None, self._reals(), self._latents, **kw)
        self.set_depth(depth)
        self.snaps = []

    def set_depth(self, depth):
        self.G.depth = self.D.depth = depth

    def _d_loss(self, D, G, real, z):
        pg.wgan_gp_loss.set_mixing_factors(torch.from_numpy(self.rs.rand(4, 1).astype(np.float32)))
        return pg.wgan_gp_D_loss(D, G, real, z)

    def _reals(self):
        while True:
            r = 4 * 2 ** int(self.G.depth)
            yield torch.from_numpy(self.rs.rand(4, 3, r, r).astype(np.float32) * 2 - 1)

    def _latents(self):
        return torch.from_numpy(self.rs.randn(4, LATENT).astype(np.float32))

    def train(self, n):
        for _ in range(n):
            self.tr.train()
            self.snaps.append(emu_ema.flat64(self.G))


def _assert_average(Gs, start, snaps, betas):
    want, bound = emu_ema.recurrence(start, snaps, betas)
    got = emu_ema.flat64(Gs)
    worst = float(np.max(np.abs(got - want) - 8 * bound))
    assert worst <= 0.0, worst
    return want


def test_average_follows_every_g_update_over_a_depth_change(emu):
    run = _Run(ema_kw=dict(beta=0.9))
    Gs = run.ema.Gs
    start = emu_ema.flat64(run.G)
    assert Gs is not run.G and Gs._flat_offsets == run.G._flat_offsets and np.array_equal(emu_ema.flat64(Gs), start)
    assert Gs._flat_param.data_ptr() != run.G._flat_param.data_ptr() and Gs._rt is not run.G._rt
    base = Gs._flat_param.data_ptr()
    assert all(base <= p.data_ptr() < base + 4 * Gs._flat_param.numel() and not p.requires_grad for p in Gs.parameters())
    run.train(2)
    run.set_depth(2)
    run.train(2)
    assert run.tr.g_ema is run.ema and run.G._rt.ema_ev is None                # (host tensors: inline, no event)
    want = _assert_average(Gs, start, run.snaps, 0.9)
    assert np.abs(want - run.snaps[-1]).max() > 1e-4                           # the average is not G: a missed update would show
    missed, _ = emu_ema.recurrence(start, run.snaps[1:], 0.9)
    assert np.abs(missed - want).max() > 1e-5
    net = run.ema.network()
    assert net is Gs and (net.depth, net.alpha) == (run.G.depth, run.G.alpha)
    assert all(p.grad is None for p in Gs.parameters())
    # a re-flatten of G (a new flat buffer, the old one released): the next update reads the new one -- shown through its contents
    run.G.float()
    with torch.no_grad():
        run.G._flat_param.add_(0.25)
    before = emu_ema.flat64(Gs)
    run.ema.update(4)
    want, bound = emu_ema.reference(before, emu_ema.flat64(run.G), 0.9)
    assert np.all(np.abs(emu_ema.flat64(Gs) - want) <= bound) and np.abs(want - before).max() > 0.02


def test_halflife_and_argument_errors(emu):
    run = _Run(ema_kw=dict(halflife_kimg=0.004))
    start = emu_ema.flat64(run.G)
    run.train(1)                                                               # minibatch 4 = one half-life
    assert run.ema.decay(4) == 0.5 and run.ema.decay(8) == 0.25
    want, bound = emu_ema.reference(start, run.snaps[0], 0.5)
    assert np.all(np.abs(emu_ema.flat64(run.ema.Gs) - want) <= bound)
    G = run.G
    with pytest.raises(ValueError):
        pg.GeneratorEMA(G, beta=0.99, halflife_kimg=10)
    for bad in (1.5, -0.1, float('nan')):
        with pytest.raises(ValueError):
            pg.GeneratorEMA(G, beta=bad)
    with pytest.raises(ValueError):
        pg.GeneratorEMA(G, halflife_kimg=0)
    other = pg.Generator(SHAPE, latent_size=LATENT, fmap_base=256, fmap_max=32)
    with pytest.raises(ValueError):
        pg.GeneratorEMA(G, Gs=other)
    with pytest.raises(ValueError):
        pg.GeneratorEMA(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError):                                            # an average of another generator than the trainer's
        _Run(trainer_kw=dict(g_ema=pg.GeneratorEMA(other)))


class _Counting(object):
    """``emu_ops`` with every function call logged by name."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        v = getattr(emu_ops, name)
        if not isinstance(v, types.FunctionType):
            return v

        def call(*a, **k):
            self._log.append(name)
            return v(*a, **k)
        return call


def _logged_run(monkeypatch, **run_kw):
    log = []
    proxy = _Counting(log)
    for modname in ('engine', 'optim', 'ema'):
        monkeypatch.setattr(importlib.import_module('pggan-pytorch_amd.' + modname), 'ops', proxy)
    run = _Run(**run_kw)
    marks = []
    for _ in range(2):
        run.tr.train()
        marks.append(len(log))
    return log, marks, run


def test_trainer_without_an_average_issues_the_ops_it_always_did(emu, monkeypatch):
    plain, _, run = _logged_run(monkeypatch)
    assert run.tr.g_ema is None and run.G._rt.ema_ev is None
    default, _, _ = _logged_run(monkeypatch, trainer_kw=dict(g_ema=None))
    assert plain and 'adam' in plain and 'ema' not in plain
    assert default == plain
    with_ema, marks, _ = _logged_run(monkeypatch, ema_kw=dict(beta=0.9))
    assert [n for n in with_ema if n != 'ema'] == plain                        # nothing else changes ...
    assert with_ema.count('ema') == 2
    assert [with_ema[m - 1] for m in marks] == ['ema', 'ema']                  # ... and the average closes each iteration,
    assert [with_ema[m - 2] for m in marks] == ['adam', 'adam']                # right behind Adam(G)


class _Z(object):
    """Latents whose ``.cuda()`` stays on the host."""

    def __init__(self, z):
        self.z = z

    def cuda(self):
        return self.z


def test_plugins_pick_the_smoothed_generator(emu):
    run = _Run(ema_kw=dict(beta=0.9))
    run.train(3)
    z = torch.from_numpy(np.random.RandomState(2).randn(2, LATENT).astype(np.float32))
    got = {}
    for smoothed in (None, True, False):
        og = pg.OutputGenerator(lambda n: _Z(z), [lambda out, kimg, s=smoothed: got.__setitem__(s, out)], samples_count=2, smoothed=smoothed)
        og.register(run.tr)
        og.epoch(1)
    gs_out, g_out = run.ema.Gs.forward(z).numpy(), run.G.forward(z).numpy()
    assert np.array_equal(got[None], gs_out) and np.array_equal(got[True], gs_out) and np.array_equal(got[False], g_out)
    assert np.abs(gs_out - g_out).max() > 1e-5
    assert run.ema.Gs.depth == run.G.depth
    plain = _Run()                                                            # no average: today's behaviour, and smoothed=True refuses
    og = pg.OutputGenerator(lambda n: _Z(z), [lambda out, kimg: got.__setitem__('plain', out)], samples_count=2)
    og.register(plain.tr)
    og.epoch(1)
    assert np.array_equal(got['plain'], plain.G.forward(z).numpy())
    for plugin in (pg.OutputGenerator(None, [], smoothed=True), pg.SWDMonitor(None, None, smoothed=True)):
        with pytest.raises(ValueError):
            plain.tr.register_plugin(plugin)
    pg.SWDMonitor(None, None, smoothed=True).register(run.tr)
    pg.SWDMonitor(None, None, smoothed=False).register(plain.tr)


def test_saver_writes_and_loader_returns_the_smoothed_generator(emu, tmp_path):
    run = _Run(ema_kw=dict(beta=0.9))
    run.train(2)
    saver = pg.SaverPlugin(str(tmp_path))
    saver.register(run.tr)
    saver.end(1)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == ['network-snapshot-%s-000000.dat' % n for n in ('discriminator', 'generator', 'generator_smoothed', 'trainer')]
    pattern = 'network-snapshot-{}-000000.dat'
    loaded = pg.load_smoothed_generator(pattern, str(tmp_path))
    assert isinstance(loaded, pg.Generator) and loaded._rt is not run.ema.Gs._rt
    assert np.array_equal(emu_ema.flat64(loaded), emu_ema.flat64(run.ema.Gs)) and loaded.depth == run.G.depth
    state = torch.load(str(tmp_path / pattern.format('trainer')), weights_only=False)
    assert state['ema_beta'] == 0.9 and state['ema_halflife_kimg'] is None
    # resume: the average goes on from the file
    G2, D2 = pg.load_models(pattern, str(tmp_path))
    resumed = _Run(seed=12, depth=int(G2.depth), ema_kw=dict(beta=0.9, Gs=loaded), G=G2, D=D2)
    assert resumed.ema.Gs is loaded
    start = emu_ema.flat64(loaded)
    resumed.train(2)
    _assert_average(loaded, start, resumed.snaps, 0.9)
    # a snapshot without one (written without an average / by an earlier version)
    saver.end(1)                                                               # (clears and rewrites: still four files)
    (tmp_path / pattern.format('generator_smoothed')).unlink()
    assert pg.load_smoothed_generator(pattern, str(tmp_path)) is None
    plain = _Run()
    other = tmp_path / 'plain'
    other.mkdir()
    saver = pg.SaverPlugin(str(other))
    saver.register(plain.tr)
    saver.end(1)
    assert sorted(p.name for p in other.iterdir()) == ['network-snapshot-%s-000000.dat' % n for n in ('discriminator', 'generator', 'trainer')]
    assert 'ema_beta' not in torch.load(str(other / pattern.format('trainer')), weights_only=False)


def test_runtime_declares_the_event_and_old_pickles_drop_it():
    assert 'ema_ev' in pg.runtime.NetRuntime.__slots__ and pg.runtime.NetRuntime().ema_ev is None
    assert '_ema_ev' in pg.runtime.LEGACY_KEYS
    G = pg.Generator(SHAPE, latent_size=LATENT, **KW)
    state = dict(G.__getstate__(), _ema_ev=None)
    G2 = pg.Generator.__new__(pg.Generator)
    G2.__setstate__(state)
    assert '_ema_ev' not in vars(G2) and G2._rt.ema_ev is None
    assert 'GeneratorEMA' in pg.__all__ and 'load_smoothed_generator' in pg.__all__
    assert pg._lib.SIGNATURES['pg_ema_f32'] == [pg._lib.P, pg._lib.P, pg._lib.L, pg._lib.F, pg._lib.P] and pg._lib.ABI_VERSION == 27
