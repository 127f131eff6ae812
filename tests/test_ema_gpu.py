"""The smoothed generator on the device: ``pg_ema_f32`` against the fp64 evaluation of its contract, and ``GeneratorEMA`` under
``Trainer`` (two streams, one stream, a torch.optim optimizer), its consumers and its checkpoint -- every average held to the fp64
recurrence over host copies of G's parameters taken after each iteration (tests/emu_ema.py: reference and derived bound)."""
import ctypes

import numpy as np
import pytest
import torch

import emu_ema
from conftest import rel_err

import pggan_amd as pg

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPE = (1, 3, 16, 16)
KW = dict(fmap_base=128, fmap_max=32)
LATENT = 32
SIZES = (1, 3, 4, 5, 1023, 1024, 4194311)      # the last: two full passes of the 2048 x 256 x 4 grid plus 7 elements (grid-stride loop and tail)


def _bits(t):
    return t.detach().cpu().view(torch.int32).clone()


@pytest.fixture(scope='module')
def operands():
    """Seeded randn operands of the largest size on the host, shared and never written: every case slices them."""
    gen = torch.Generator().manual_seed(1234)
    n = max(SIZES)
    return torch.randn(n + 8, generator=gen), torch.randn(n, generator=gen)


@pytest.mark.parametrize('n', SIZES)
def test_kernel_against_fp64(operands, n):
    avg0, p0 = operands[0][:n + 8].to(DEV), operands[1][:n].to(DEV)
    a64, p64 = avg0[:n].cpu().double().numpy(), p0.cpu().double().numpy()
    p_bits = _bits(p0)
    for beta in (0.999, 0.5, 0.0):
        avg = avg0.clone()
        pg.ops.ema(avg[:n], p0, beta)
        torch.cuda.synchronize()
        want, bound = emu_ema.reference(a64, p64, beta)
        err = np.abs(avg[:n].cpu().double().numpy() - want)
        print('n %d beta %g: max err %.3e, max err / bound %.3f' % (n, beta, err.max(), float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(err <= bound), (n, beta, float((err - bound).max()))
        assert torch.equal(_bits(avg[n:]), _bits(avg0[n:]))                 # the eight elements behind the range
        assert torch.equal(_bits(p0), p_bits)
    avg = avg0.clone()
    pg.ops.ema(avg[:n], p0, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(avg), _bits(avg0)) and torch.equal(_bits(p0), p_bits)


def test_argument_errors_launch_nothing():
    avg, p = torch.randn(64, device=DEV), torch.randn(64, device=DEV)
    before = _bits(avg)
    s = torch.cuda.current_stream().cuda_stream
    a, q = avg.data_ptr(), p.data_ptr()
    cases = [((None, q, 64, 0.5), 'PG_E_ARG'), ((a, None, 64, 0.5), 'PG_E_ARG'), ((a, q, 0, 0.5), 'PG_E_ARG'),
             ((a + 4, q, 32, 0.5), 'PG_E_ALIGN'), ((a, q + 4, 32, 0.5), 'PG_E_ALIGN'),
             ((a, q, 64, 1.5), 'PG_E_ARG'), ((a, q, 64, -0.1), 'PG_E_ARG'), ((a, q, 64, float('nan')), 'PG_E_ARG'),
             ((a, a + 16, 32, 0.5), 'PG_E_ARG'), ((a + 16, a, 32, 0.5), 'PG_E_ARG'), ((a, a, 64, 0.5), 'PG_E_ARG')]
    for args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            pg._lib.call('pg_ema_f32', *(args + (ctypes.c_void_p(s),)))
    pg._lib.call('pg_ema_f32', a, a + 128, 32, 0.5, ctypes.c_void_p(s))      # adjacent halves of one buffer do not overlap
    torch.cuda.synchronize()
    assert torch.equal(_bits(avg)[32:], before[32:]) and not torch.equal(_bits(avg)[:32], before[:32])
    with pytest.raises(ValueError):
        pg.ops.ema(avg, p[:32], 0.5)
    with pytest.raises(ValueError):
        pg.ops.ema(avg.cpu(), p.cpu(), 0.5)


class _Run(object):
    """A narrow 16x16 pair under Trainer on the device, minibatch 4, FusedAdam lr 1e-3, growth stage set by hand."""

    def __init__(self, seed=11, depth=1, ema_kw=None, G=None, D=None, torch_adam=False):
        torch.manual_seed(seed)
        self.G = G if G is not None else pg.Generator(SHAPE, latent_size=LATENT, **KW).to(DEV)
        self.D = D if D is not None else pg.Discriminator(SHAPE, **KW).to(DEV)
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.ema = None if ema_kw is None else pg.GeneratorEMA(self.G, **ema_kw)
        opt_g = (torch.optim.Adam if torch_adam else pg.FusedAdam)(self.G.parameters(), 0.001, betas=(0.0, 0.99))
        opt_d = pg.FusedAdam(self.D.parameters(), 0.001, betas=(0.0, 0.99))
        kw = {} if self.ema is None else dict(g_ema=self.ema)
        self.tr = pg.Trainer(self.D, self.G, pg.wgan_gp_D_loss, pg.wgan_gp_G_loss, opt_d, opt_g, None, self._reals(), self._latents, **kw)
        self.G.depth = self.D.depth = depth
        self.snaps = []

    def _reals(self):
        while True:
            r = 4 * 2 ** int(self.G.depth)
            yield torch.rand((4, 3, r, r), device=DEV, generator=self.gen) * 2 - 1

    def _latents(self):
        return torch.randn((4, LATENT), device=DEV, generator=self.gen)

    def train(self, n):
        for _ in range(n):
            self.tr.train()
            self.snaps.append(emu_ema.flat64(self.G))                        # (synchronises)


def _assert_average(Gs, start, snaps, betas, what=''):
    want, bound = emu_ema.recurrence(start, snaps, betas)
    err = np.abs(emu_ema.flat64(Gs) - want)
    print('%s: %d elements, max err %.3e, max err / (8 x step bound) %.3f'
          % (what, err.size, err.max(), float(np.max(err / np.maximum(8 * bound, 1e-300)))))
    assert np.all(err <= 8 * bound), float((err - 8 * bound).max())
    return want


@pytest.mark.parametrize('mode', ['two_streams', 'one_stream', 'torch_adam'])
def test_trainer_average_matches_the_recurrence(mode, deterministic_forward, monkeypatch):
    """Eight iterations with a depth change 1 -> 2 after the fourth; beta = 0.9, so that a missed or doubled update (or one that read G's
    parameters while Adam was writing them) is far outside round-off.  Not-yet-grown blocks and retired toRGB layers are part of the
    comparison: the whole flat buffer."""
    if mode == 'one_stream':
        monkeypatch.setattr(pg.engine, 'ASYNC_WGRAD', False)
    run = _Run(ema_kw=dict(beta=0.9), torch_adam=(mode == 'torch_adam'))
    Gs = run.ema.Gs
    start = emu_ema.flat64(run.G)
    assert Gs._flat_offsets == run.G._flat_offsets and np.array_equal(emu_ema.flat64(Gs), start)
    assert Gs._flat_param.data_ptr() != run.G._flat_param.data_ptr() and not any(p.requires_grad for p in Gs.parameters())
    run.train(4)
    run.G.depth = run.D.depth = 2
    run.train(4)
    assert (run.G._rt.ema_ev is None) == (mode == 'one_stream')               # the second-stream placement was really taken (or not)
    want = _assert_average(Gs, start, run.snaps, 0.9, mode)
    missed, _ = emu_ema.recurrence(start, run.snaps[:-1], 0.9)
    assert np.abs(missed - want).max() > 1e-5                                  # (what a dropped update would look like: 1e4 x the bound)
    assert all(p.grad is None for p in Gs.parameters()) and Gs._flat_grad is None


def test_halflife_in_images(deterministic_forward):
    run = _Run(ema_kw=dict(halflife_kimg=0.004))
    start = emu_ema.flat64(run.G)
    run.train(1)                                                               # minibatch 4 = one half-life: Gs moves exactly halfway
    want, bound = emu_ema.reference(start, run.snaps[0], 0.5)
    err = np.abs(emu_ema.flat64(run.ema.Gs) - want)
    print('halflife: max err %.3e, max err / bound %.3f' % (err.max(), float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(err <= bound)
    assert np.abs(run.snaps[0] - start).max() > 1e-4
    with pytest.raises(ValueError):
        pg.GeneratorEMA(run.G, beta=0.99, halflife_kimg=10)


def test_consumers_evaluate_the_smoothed_generator(deterministic_forward):
    run = _Run(depth=2, ema_kw=dict(beta=0.9))
    run.train(3)
    z = torch.randn((3, LATENT), generator=torch.Generator().manual_seed(5))
    got = {}
    for smoothed in (None, False):
        og = pg.OutputGenerator(lambda n: z.clone(), [lambda out, kimg, s=smoothed: got.__setitem__(s, out)], samples_count=3, smoothed=smoothed)
        run.tr.register_plugin(og)
        og.epoch(1)
    gs_out, g_out = run.ema.Gs.forward(z.to(DEV)).clone(), run.G.forward(z.to(DEV)).clone()     # (a later pass may reuse the output buffer)
    assert got[None].shape == (3, 3, 16, 16)
    print('consumers: Gs %.3e, G %.3e, Gs vs G %.3e' % (rel_err(got[None], gs_out), rel_err(got[False], g_out), rel_err(gs_out, g_out)))
    assert rel_err(got[None], gs_out) < 1e-5 and rel_err(got[False], g_out) < 1e-5
    assert rel_err(got[None], g_out) > 1e-4                                    # not the raw generator's
    plain = _Run()
    for plugin in (pg.SWDMonitor(None, None, smoothed=True), pg.OutputGenerator(None, [], smoothed=True)):
        with pytest.raises(ValueError):
            plain.tr.register_plugin(plugin)
    # SWDMonitor: the fake batches come from Gs
    seen = []
    swd = pg.SWDMonitor(lambda n: torch.rand((n, 3, 16, 16), device=DEV) * 2 - 1, lambda n: z[:n].clone(), num_images=3, minibatch=3,
                        patches_per_image=8)
    run.tr.register_plugin(swd)
    feed = pg.metrics.SlicedWasserstein.feed_fake
    try:
        pg.metrics.SlicedWasserstein.feed_fake = lambda self, x: (seen.append(x.clone()), feed(self, x))[1]
        swd.epoch(1)
    finally:
        pg.metrics.SlicedWasserstein.feed_fake = feed
    assert len(seen) == 1 and rel_err(seen[0], gs_out) < 1e-5 and 'swd' in run.tr.stats


def test_checkpoint_resume_and_generate(deterministic_forward, tmp_path):
    run = _Run(ema_kw=dict(beta=0.9))
    run.train(3)
    saver = pg.SaverPlugin(str(tmp_path))
    run.tr.register_plugin(saver)
    saver.end(1)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == ['network-snapshot-%s-000000.dat' % n for n in ('discriminator', 'generator', 'generator_smoothed', 'trainer')]
    pattern = 'network-snapshot-{}-000000.dat'
    loaded = pg.load_smoothed_generator(pattern, str(tmp_path))
    assert torch.equal(_bits(loaded._flat_param), _bits(run.ema.Gs._flat_param)) and loaded.depth == run.G.depth
    empty = tmp_path / 'empty'
    empty.mkdir()
    assert pg.load_smoothed_generator(pattern, str(empty)) is None
    state = torch.load(str(tmp_path / pattern.format('trainer')), weights_only=False)
    assert state['ema_beta'] == 0.9 and state['ema_halflife_kimg'] is None
    got = []
    out = pg.utils.output_samples(str(tmp_path / pattern.format('generator_smoothed')), 2, [lambda o, d: got.append(o)], 'smoothed')
    assert got[0].shape == (2, 3, 8, 8) and bool(torch.isfinite(out).all())              # (the snapshot carries its growth stage: depth 1)
    # resume: two more iterations on the reloaded pair continue the reloaded average
    G2, D2 = pg.load_models(pattern, str(tmp_path))
    resumed = _Run(seed=12, depth=int(G2.depth), ema_kw=dict(beta=0.9, Gs=loaded), G=G2, D=D2)
    assert resumed.ema.Gs is loaded
    start = emu_ema.flat64(loaded)
    assert np.array_equal(start, emu_ema.flat64(run.ema.Gs))
    resumed.train(2)
    want = _assert_average(loaded, start, resumed.snaps, 0.9, 'resumed')
    from_g, _ = emu_ema.recurrence(emu_ema.flat64(run.G), resumed.snaps, 0.9)
    assert np.abs(from_g - want).max() > 1e-5                                  # (an average restarted from G is something else)
    with pytest.raises(ValueError):
        pg.GeneratorEMA(run.G, Gs=pg.Generator(SHAPE, latent_size=LATENT, fmap_base=256, fmap_max=32).to(DEV))
