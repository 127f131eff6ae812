"""Device tier of the differentiable augmentation: the four kernels of csrc/augment.hip against the numpy twin with ``==``, the D and G steps
with injected tables against float64 autograd through the oracle's networks (tests/augment_ref.py), the identity twin, eager | plan |
hipGraph replay with a table per step, and three Trainer iterations under an AugmentController."""
import numpy as np
import pytest
import torch

import augment_ref as ar
from conftest import fixture_params, load_fixture, rel_err
from helpers import assert_same_contributions, build_nets, grads_by_name, load_fixture_params, reference_grads, synthetic
from test_e2e_gpu import GRAD_TOL, OUT_TOL          # the bounds test_golden_fixture applies to WGAN-GP on tiny32 / tiny16c1

import pggan_amd as pg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
A = pg.augment


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want, what):
    got, want = ar.bits(got.cpu().numpy()), ar.bits(want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, '%s: %d elements differ, first at %s: %#x, twin %#x' % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the gather and its transpose -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', [4, 8, 16, 64])
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('N', [1, 3, 16])
def test_apply_and_adjoint_are_the_twin(N, C, W):
    """Every row of the hand-made pool (every dx mod 4, dx = +-(W - 1), +-W, both flips, cutouts at each edge, gain rows, the identity), N
    rows per launch, on images with -0.0 and denormals planted in every plane."""
    H = W
    x, g = ar.images(N, C, H, W, seed=W + C), ar.images(N, C, H, W, seed=100 + W + C)
    xd, gd = _dev(x), _dev(g)
    pool = ar.pool(H, W)
    pool = np.concatenate([pool, pool[:(-len(pool)) % N]])                     # (whole launches of N rows)
    assert len(pool) % N == 0
    mask = (1 << C) - 1 if N == 3 else 1
    for k in range(0, len(pool), N):
        table = pool[k:k + N]
        td = _dev(table)
        _same_bits(pg.ops.augment_apply(xd, td, mask), A.apply_host(x, table, mask), 'apply, rows %d..' % k)
        _same_bits(pg.ops.augment_adjoint(gd, td), A.adjoint_host(g, table), 'adjoint, rows %d..' % k)
    # an identity table is a bit copy, -0.0 and denormals included; out= is written in place
    out = torch.full_like(xd, float('nan'))
    assert pg.ops.augment_apply(xd, torch.zeros((N, 8), dtype=torch.int32, device=DEV), mask, out=out) is out
    _same_bits(out, x, 'identity')


def test_apply_and_adjoint_past_the_grid_cap():
    """2 x 3 x 1024^2: 1.5 M threads' worth of work on a grid capped at 4096 x 256."""
    N, C, H, W = 2, 3, 1024, 1024
    rs = np.random.RandomState(7)
    x = rs.randn(N, C, H, W).astype(np.float32)
    table = np.asarray([ar.row(flip=1, dy=-37, dx=1021, y0=100, y1=611, x0=0, x1=333, gain=0.125),
                        ar.row(flip=0, dy=513, dx=-258, y0=0, y1=1024, x0=1000, x1=1024)], dtype=np.int32)
    xd, td = _dev(x), _dev(table)
    _same_bits(pg.ops.augment_apply(xd, td, 0b101), A.apply_host(x, table, 0b101), 'apply')
    _same_bits(pg.ops.augment_adjoint(xd, td), A.adjoint_host(x, table), 'adjoint')


def test_augmenter_methods_are_the_kernels():
    aug = pg.Augmenter(gain=0.5, gain_channels=(1,), device=DEV)
    x = ar.images(3, 2, 8, 8, seed=1)
    table = ar.pool(8, 8)[-6:-3]
    y = aug.apply(_dev(x), _dev(table))
    _same_bits(y, A.apply_host(x, table, 0b10), 'Augmenter.apply')
    _same_bits(aug.adjoint(y, _dev(table)), A.adjoint_host(y.cpu().numpy(), table), 'Augmenter.adjoint')


def test_argument_errors():
    x = torch.zeros((2, 1, 8, 8), device=DEV)
    t = torch.zeros((2, 8), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        pg.ops.augment_apply(x, t[:1])
    with pytest.raises(ValueError):
        pg.ops.augment_apply(x, t.float())
    with pytest.raises(pg.ops.Unsupported):
        pg.ops.augment_apply(torch.zeros((2, 1, 6, 8), device=DEV), t)
    with pytest.raises(pg.ops.Unsupported):
        pg.ops.augment_adjoint(torch.zeros((2, 1, 8, 2), device=DEV), t)
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg.ops.augment_apply(x, t, out=x)                                          # a gather cannot run in place
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg.ops.augment_apply(torch.zeros((2, 33, 4, 4), device=DEV), t)
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):
        pg.ops.augment_apply(torch.zeros(2 * 64 + 1, device=DEV)[1:].view(2, 1, 8, 8), t)
    U = torch.zeros((2, 8), device=DEV)
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg.ops.augment_table(U, 8, 8, 0.0, 1.5, 0.0, 0.0, 0.0, False, 1.0)
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg.ops.augment_table(U, 8, 8, 0.0, 0.0, 0.0, 0.0, -1.0, False, 1.0)
    with pytest.raises(pg.ops.Unsupported):
        pg.ops.augment_table(U, 8, 12, 0.0, 0.0, 0.0, 0.0, 0.0, False, 1.0)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg.ops.score_signs(torch.zeros(pg.ops.AUGMENT_MAX_SCORES + 1, device=DEV), acc)
    with pytest.raises(ValueError):
        pg.ops.score_signs(torch.zeros(3, device=DEV), acc.float())


# ---- the table and the sign count -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,H,W', [(1, 4, 4), (7, 16, 64), (300, 1024, 1024), (257, 64, 8)])
@pytest.mark.parametrize('p', [0.0, 0.37, 1.0])
def test_table_kernel_is_the_twin(rows, H, W, p):
    for k, kw in enumerate((dict(translate=(0.125, 0.125), cutout=(0.5, 0.5), gain=0.25, flip=True),
                            dict(translate=(1.0, 0.3), cutout=(1.0, 0.1), gain=2.0),
                            dict(translate=(0.0, 1.0), cutout=(0.07, 1.0), flip=True), dict())):
        aug, twin = pg.Augmenter(p=p, seed=50 + k, device=DEV, **kw), pg.Augmenter(p=p, seed=50 + k, device='cpu', **kw)
        for which in ('d', 'g', 'd'):
            got, want = aug.table(rows, H, W, which), twin.table(rows, H, W, which)
            assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got.cpu(), want), (kw, which, got.cpu()[:4], want[:4])
        assert aug.draws == twin.draws == {'d': 2, 'g': 1}
    # ... and on draws at the edges of [0, 1): 0 and the largest float32 below 1 in every column
    U = np.stack([np.zeros(8, np.float32), np.full(8, 1 - 2.0 ** -24, np.float32), np.full(8, 0.5, np.float32), np.full(8, 0.5 - 2.0 ** -25, np.float32)])
    got = pg.ops.augment_table(_dev(U), H, W, 1.0, 1.0, 0.5, 0.5, 1.0, True, p)
    assert np.array_equal(got.cpu().numpy(), A.table_host(U, H, W, 1.0, 1.0, 0.5, 0.5, 1.0, True, p))


@pytest.mark.parametrize('n', [1, 3, 16, 65])
def test_score_signs_is_numpy(n):
    rs = np.random.RandomState(n)
    s = rs.randn(n).astype(np.float32)
    s[::3] = 0.0
    s[1::7] = -0.0
    s[n // 2] = 1e-42                                                            # a positive denormal counts as positive
    acc = torch.tensor([5.0, 7.0], dtype=torch.float64, device=DEV)
    assert pg.ops.score_signs(_dev(s), acc) is acc
    want = [5.0 + float(np.sign(s.astype(np.float64)).sum()), 7.0 + n]
    assert acc.cpu().tolist() == want
    pg.ops.score_signs(_dev(-s), acc)                                            # accumulates: the opposite signs cancel the first call
    assert acc.cpu().tolist() == [5.0, 7.0 + 2 * n]


# ---- the steps against float64 autograd -------------------------------------------------------------------------------------------------
_nets = {}


def _fixture_nets(name):
    if name not in _nets:
        meta, data = load_fixture(name)
        G, D = build_nets(meta, DEV)
        load_fixture_params(G, data, 'G')
        load_fixture_params(D, data, 'D')
        c = meta['cfg']
        cfg = ar.oc.NetCfg(c['resolution'], c['num_channels'], fmap_base=c['fmap_base'], fmap_decay=c['fmap_decay'], fmap_max=c['fmap_max'],
                           latent_size=c['latent_size'])
        _nets[name] = (meta, G, D, fixture_params(data, 'G'), fixture_params(data, 'D'), cfg)
    return _nets[name]


def _step_case(kind, penalty, name, alpha, seed, n):
    """Inputs, tables and the float64 reference of one case (the reference is computed once and shared with the control)."""
    meta, G, D, gp, dp, cfg = _fixture_nets(name)
    depth, r = cfg.max_depth, cfg.resolution
    drift = 0.001 if kind == 'wgan' else 0.0
    real, z_d, z_g, mix = synthetic(seed + n, n, cfg.num_channels, r, cfg.latent_size)
    td, tg = ar.step_table(2 * n, r, r, seed), ar.step_table(n, r, r, seed + 1)
    want = ar.d_loss_and_grads(dp, gp, cfg, real, z_d, mix, depth, alpha, kind, drift, penalty, 10.0, td, 1)
    gwant = ar.g_loss_and_grads(gp, dp, cfg, z_g, depth, alpha, kind, tg, 1)
    return (real, z_d, z_g, mix), (td, tg), want, gwant


@pytest.mark.parametrize('n', [3, 4])
@pytest.mark.parametrize('name,alpha,seed', [('tiny16c1', 1.0, 21), ('tiny16c1', 0.5, 22), ('tiny32', 1.0, 23), ('tiny32', 0.5, 24)])
@pytest.mark.parametrize('kind,penalty', [('logistic', 'r1'), ('hinge', None), ('wgan', 'gp')])
def test_augmented_steps_against_float64_oracle(kind, penalty, name, alpha, seed, n):
    """``test_objectives_against_float64_oracle`` of tests/test_gan_losses_gpu.py with an Augmenter and injected tables that shift, flip,
    cut and gain: losses and every gradient of D and of G (the G gradients pass through the transpose) at that test's bounds."""
    meta, G, D, gp, dp, cfg = _fixture_nets(name)
    G.depth = D.depth = cfg.max_depth
    G.alpha = D.alpha = alpha
    (real, z_d, z_g, mix), (td, tg), want, gwant = _step_case(kind, penalty, name, alpha, seed, n)
    if kind == 'hinge':            # a condition on the inputs, not a tolerance: no score within 1e-3 of a kink
        assert float((1 - want['s_r']).abs().min()) > 1e-3 and float((1 + want['s_f']).abs().min()) > 1e-3
    aug = pg.Augmenter(gain=0.3, gain_channels=(0,), device=DEV)
    D_loss, G_loss = pg.gan_losses(kind, penalty=penalty, penalty_weight=10.0, augment=aug)
    pg.wgan_gp_loss.enable_graphs(False)                                        # eagerly
    if penalty == 'gp':
        pg.wgan_gp_loss.set_mixing_factors(mix)
    aug.inject(d_table=td, g_table=tg)
    d_cost, d_real, d_fake = D_loss(D, G, real.to(DEV), z_d.to(DEV))
    errs = dict(d_cost=rel_err(d_cost, want['d_cost']), R=rel_err(d_real, want['R']), F=rel_err(d_fake, want['F']))
    d_cost.backward()
    mine = reference_grads(D)
    assert sorted(mine) == sorted(want['grads']), 'active-parameter set differs'
    derr = {k: ar.go.grad_err(k, mine[k], r, want['bias_terms']) for k, r in want['grads'].items()}
    g_cost = G_loss(G, D, z_g.to(DEV))
    errs['g_cost'] = rel_err(g_cost, gwant['g_cost'])
    g_cost.backward()
    mine = reference_grads(G)
    assert sorted(mine) == sorted(gwant['grads'])
    gerr = {k: rel_err(mine[k], r) for k, r in gwant['grads'].items()}
    print('%s/%s %s alpha %g n %d: losses %s, worst D gradient %.2e, worst G gradient %.2e'
          % (kind, penalty, name, alpha, n, {k: '%.1e' % v for k, v in errs.items()}, max(derr.values()), max(gerr.values())))
    assert aug.draws == {'d': 0, 'g': 0}                                        # the injected tables were used, nothing was drawn
    assert all(v < OUT_TOL for v in errs.values()), errs
    assert all(v < GRAD_TOL for v in derr.values()), max((v, k) for k, v in derr.items())
    assert all(v < GRAD_TOL for v in gerr.values()), max((v, k) for k, v in gerr.items())


def test_without_the_transpose_the_g_gradients_miss_the_bound(monkeypatch):
    """Control of the test above: the identity in ``augment_adjoint``'s place, and the G gradients exceed GRAD_TOL."""
    kind, penalty, name, alpha, seed, n = 'logistic', 'r1', 'tiny32', 1.0, 23, 4
    meta, G, D, gp, dp, cfg = _fixture_nets(name)
    G.depth = D.depth = cfg.max_depth
    G.alpha = D.alpha = alpha
    (real, z_d, z_g, mix), (td, tg), want, gwant = _step_case(kind, penalty, name, alpha, seed, n)
    aug = pg.Augmenter(gain=0.3, gain_channels=(0,), device=DEV)
    _, G_loss = pg.gan_losses(kind, penalty=penalty, penalty_weight=10.0, augment=aug)
    pg.wgan_gp_loss.enable_graphs(False)
    monkeypatch.setattr(pg.ops, 'augment_adjoint', lambda g, table, out=None: g)
    aug.inject(g_table=tg)
    g_cost = G_loss(G, D, z_g.to(DEV))
    assert rel_err(g_cost, gwant['g_cost']) < OUT_TOL                           # the forward is untouched
    g_cost.backward()
    mine = reference_grads(G)
    gerr = {k: rel_err(mine[k], r) for k, r in gwant['grads'].items()}
    print('worst G gradient without the transpose: %.2e' % max(gerr.values()))
    assert max(gerr.values()) > GRAD_TOL


# ---- the identity twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,penalty', [('logistic', 'r1'), ('hinge', None)])
def test_p_zero_is_the_unaugmented_step(deterministic_forward, kind, penalty):
    """``Augmenter(p=0)`` against the same objective without one: identity rows copy bits, so the losses are ``==``; the gradients within
    the plan-versus-eager twin bounds of test_plain_schedule_matches_wgan_gp_with_lambda_zero (per tensor 1e-2, whole buffer 2e-4: the
    weight gradients commit with atomics)."""
    meta, G, D, _, _, cfg = _fixture_nets('tiny32')
    G.depth = D.depth = cfg.max_depth
    G.alpha = D.alpha = 1.0
    real, z_d, z_g, _ = synthetic(31, 4, 3, 32, cfg.latent_size)
    real, z_d, z_g = real.to(DEV), z_d.to(DEV), z_g.to(DEV)
    pg.wgan_gp_loss.enable_graphs(False)
    aug = pg.Augmenter(p=0.0, translate=(0.25, 0.25), cutout=(0.5, 0.5), gain=0.5, flip=True, device=DEV)
    out = []
    for pair in (pg.gan_losses(kind, penalty=penalty, augment=aug), pg.gan_losses(kind, penalty=penalty)):
        c = pair[0](D, G, real, z_d)
        c[0].backward()
        gd = grads_by_name(D)
        g = pair[1](G, D, z_g)
        g.backward()
        out.append((c, gd, g, grads_by_name(G)))
    (ca, gda, ga, gga), (cb, gdb, gb, ggb) = out
    assert aug.draws == {'d': 1, 'g': 1}
    assert float(ca[0]) == float(cb[0]) and torch.equal(ca[1], cb[1]) and torch.equal(ca[2], cb[2]) and float(ga) == float(gb)
    assert_same_contributions(gda, gdb, tol=1e-2, total=2e-4)
    assert_same_contributions(gga, ggb, tol=1e-2, total=2e-4)


# ---- replay -----------------------------------------------------------------------------------------------------------------------------
def test_replayed_steps_read_their_table(deterministic_forward):
    """Eager, launch-plan and hipGraph steps with injected tables agree (cost 1e-6, gradient buffers 2e-4 rel. L2: the bounds of
    test_r1_replays_from_a_plan_of_its_own); a replay with another table gives another loss -- the table is an input of the step, not
    part of the recording -- and a new ``p`` records nothing."""
    wl, plans = pg.wgan_gp_loss, pg.plans
    torch.manual_seed(21)
    shape, kw = (1, 3, 32, 32), dict(fmap_base=512, fmap_max=64)
    G, D = pg.Generator(shape, latent_size=64, **kw).cuda(), pg.Discriminator(shape, **kw).cuda()
    G.depth = D.depth = 3
    n = 6
    gen = torch.Generator(device='cuda').manual_seed(9)
    real = torch.rand((n, 3, 32, 32), device=DEV, generator=gen) * 2 - 1
    z, zg = torch.randn((n, 64), device=DEV, generator=gen), torch.randn((n, 64), device=DEV, generator=gen)
    tables = [(ar.step_table(2 * n, 32, 32, s), ar.step_table(n, 32, 32, s + 1)) for s in (1, 5)]
    aug = pg.Augmenter(gain=0.3, device=DEV)
    pg.AugmentController(aug)                                                   # (the sign count rides in the recorded step)
    D_loss, G_loss = pg.gan_losses('logistic', penalty='r1', augment=aug)

    def l2(a, b):
        return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))

    def step(which):
        aug.inject(*tables[which])
        c = D_loss(D, G, real, z)[0]
        c.backward()
        dg = D._flat_grad.clone()
        g = G_loss(G, D, zg)
        g.backward()
        torch.cuda.synchronize()
        return float(c), dg, float(g), G._flat_grad.clone()
    wl.enable_graphs(False)
    plans.STATS.update(recorded=0, replayed=0)
    try:
        eager = [step(0), step(1)]
        assert abs(eager[0][0] - eager[1][0]) > 1e-3 * abs(eager[0][0]) and abs(eager[0][2] - eager[1][2]) > 1e-3 * abs(eager[0][2])
        counted = aug.read()
        assert counted[1] == 2 * n
        for mode in ('auto', True):
            wl._use_graphs = mode
            for _ in range(3):                                                  # two eager warm-ups, the recorded (captured) step
                step(0)
            for which in (0, 1, 0):                                             # replays
                got, want = step(which), eager[which]
                print('%s table %d: d_cost %.9g | %.9g, g_cost %.9g | %.9g, D gradients %.2e, G gradients %.2e'
                      % (mode, which, got[0], want[0], got[2], want[2], l2(got[1], want[1]), l2(got[3], want[3])))
                assert abs(got[0] - want[0]) <= 1e-6 * max(1.0, abs(want[0])) and abs(got[2] - want[2]) <= 1e-6 * max(1.0, abs(want[2])), (mode, which)
                assert l2(got[1], want[1]) < 2e-4 and l2(got[3], want[3]) < 2e-4, (mode, which)
            if mode == 'auto':
                assert plans.STATS == dict(recorded=2, replayed=2 * 3), plans.STATS
                aug.p = 0.25                                                    # a new p: drawn tables, the same plans
                for _ in range(2):
                    D_loss(D, G, real, z)[0].backward()
                    G_loss(G, D, zg).backward()
                torch.cuda.synchronize()
                assert plans.STATS == dict(recorded=2, replayed=2 * 5) and aug.draws == {'d': 2, 'g': 2}, (plans.STATS, aug.draws)
                aug.p = 1.0
            else:
                assert len(pg.graphs._CACHE) == 2 and all(g.graph is not None for g in pg.graphs._CACHE.values())
        # every D step, eager, warm-up, recorded or replayed, counted its n real scores
        assert aug.read()[1] == counted[1] + n * (6 + 2 + 6)
    finally:
        wl.enable_graphs(False)


# ---- Trainer ----------------------------------------------------------------------------------------------------------------------------
def test_trainer_iterations_under_the_controller():
    wl = pg.wgan_gp_loss
    meta, data = load_fixture('tiny16c1')
    G, D = build_nets(meta, DEV)
    load_fixture_params(G, data, 'G')
    load_fixture_params(D, data, 'D')
    G.depth = D.depth = 2
    c = meta['cfg']
    opt_g = pg.FusedAdam(G.parameters(), 0.001, betas=(0.0, 0.99))
    opt_d = pg.FusedAdam(D.parameters(), 0.001, betas=(0.0, 0.99))
    ds = pg.utils.SyntheticDataset(16, 1, seed=5)
    ds.model_depth = 2
    aug = pg.Augmenter(p=0.4, translate=(0.125, 0.125), cutout=(0.25, 0.25), gain=0.2, flip=True, seed=11, device=DEV)
    D_loss, G_loss = pg.gan_losses('logistic', penalty='r1', augment=aug)
    tr = pg.Trainer(D, G, D_loss, G_loss, opt_d, opt_g, ds, ds.loader(4), pg.utils.device_latents(4, c['latent_size'], seed=3))
    ctl = pg.AugmentController(aug, target=0.6, adjust_kimg=0.05, interval=1, p_max=0.8)      # 4 images move p by 0.08
    tr.register_plugin(ctl)
    seen = []

    class Rec(pg.Plugin):
        def __init__(self):
            super(Rec, self).__init__([(1, 'iteration')])

        def register(self, trainer):
            pass

        def iteration(self, i, g_cost, d_cost, d_real, d_fake):
            seen.append((float(g_cost), float(d_cost), tr.stats['augment_p']['val'], tr.stats['augment_rt']['val'], aug.p))
    tr.register_plugin(Rec())
    wl.enable_graphs('auto')
    try:
        p = aug.p
        for _ in range(3):
            tr.train()
        torch.cuda.synchronize()
        assert len(seen) == 3 and np.all(np.isfinite(seen)), seen
        for g_cost, d_cost, stat_p, r_t, now in seen:
            assert stat_p == now and 0.0 <= now <= 0.8 and -1.0 <= r_t <= 1.0 and r_t * 4 == round(r_t * 4)      # a mean of 4 signs
            step = (r_t > 0.6) - (r_t < 0.6)
            assert now == min(max(p + step * 4 / (1000.0 * 0.05), 0.0), 0.8) and (step == 0 or now != p or p in (0.0, 0.8)), (p, r_t, now)
            p = now
        assert aug.read()[1] == 12 and aug.draws == {'d': 3, 'g': 3}
    finally:
        wl.enable_graphs(False)
