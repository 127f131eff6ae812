"""Selectable GAN objectives on the MI355X: the three kernels of csrc/gan_losses.hip against the fp64 references and
derived bounds of tests/gan_losses_ref.py; the objectives end to end through the public interface against float64 autograd through the
oracle's networks; the no-penalty schedule against its WGAN twin; launch-plan replay; three Trainer iterations."""
import numpy as np
import pytest
import torch

import gan_losses_oracle as go
import gan_losses_ref as ref
from conftest import fixture_params, load_fixture, rel_err
from helpers import assert_same_contributions, build_nets, grads_by_name, load_fixture_params, reference_grads, synthetic
from test_e2e_gpu import GRAD_TOL, OUT_TOL          # the bounds test_golden_fixture applies to WGAN-GP on tiny32 / tiny16c1

import pggan_amd as pg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KINDS = ref.KINDS
ops = pg.ops


def _scores(n, seed):
    """Normal draws scaled by 3 with the fixed set (+-0, +-1 and their fp32 neighbours, +-30, +-100, +-1e4) in front, as far as it fits."""
    rs = np.random.RandomState(seed)
    s = (rs.randn(n) * 3).astype(np.float32)
    k = min(n, ref.FIXED_SCORES.size)
    s[:k] = np.roll(ref.FIXED_SCORES, seed)[:k]
    return s


def _within(got, want, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(-1)
    want, bound = np.asarray(want, np.float64).reshape(-1), np.broadcast_to(np.asarray(bound, np.float64).reshape(-1), got.shape)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
    print('%s: largest error / bound %.3f' % (what, worst))
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(err <= bound), (what, worst)


# ---- the loss-block kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 3, 16, 64, 65, 1000])
@pytest.mark.parametrize('kind', KINDS)
def test_loss_kernels_within_derived_bounds(kind, N):
    drift = 0.001 if kind == 'wgan' else 0.0
    for groups, with_pen, drift_ in ((2, False, drift), (3, True, drift), (3, False, 0.25), (2, True, 0.0)):
        s = np.concatenate([_scores(N, N), _scores(N, N + 3), np.random.RandomState(N).randn((groups - 2) * N).astype(np.float32)])
        pen = np.random.RandomState(N + 1).rand(N).astype(np.float32) * 4 if with_pen else None
        s_d = torch.from_numpy(s).to(DEV)
        pen_d = torch.from_numpy(pen).to(DEV) if with_pen else None
        got = ops.gan_d_loss(s_d, pen_d, N, kind, drift_)
        again = ops.gan_d_loss(s_d, pen_d, N, kind, drift_)
        want = ref.gan_d_loss(s, pen, N, groups, kind, drift_)
        tag = '%s N=%d groups=%d pen=%s drift=%g' % (kind, N, groups, with_pen, drift_)
        assert tuple(got[1].shape) == tuple(got[2].shape) == (N, 1) and got[3].numel() == groups * N
        assert got[0]._base is got[1]._base is got[2]._base and got[0]._base is not None          # views of ONE buffer (plans.d_step clones it once)
        for a, b, name in zip(got, again, ('d_cost', 'd_real', 'd_fake', 'gscore')):
            _within(a, want[name][0], want[name][1], tag + ' ' + name)
            assert torch.equal(a.view(-1).view(torch.int32), b.view(-1).view(torch.int32)), (tag, name, 'bits differ between two calls')
        if groups == 3:
            assert not bool(got[3][2 * N:].any())
    s = _scores(N, N + 7)
    s_d = torch.from_numpy(s).to(DEV)
    c, gs = ops.gan_g_loss(s_d, kind)
    c2, gs2 = ops.gan_g_loss(s_d, kind)
    wc, ec, wg, eg = ref.gan_g_loss(s, kind)
    _within(c, wc, ec, '%s N=%d g_cost' % (kind, N))
    _within(gs, wg, eg, '%s N=%d g gscore' % (kind, N))
    assert torch.equal(c.view(1).view(torch.int32), c2.view(1).view(torch.int32)) and torch.equal(gs.view(torch.int32), gs2.view(torch.int32))


def test_hinge_derivative_is_zero_at_the_kink():
    one = np.float32(1)
    sr = np.array([1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), -1.0, 0.0], np.float32)
    sf = np.array([-1.0, np.nextafter(-one, np.float32(0)), np.nextafter(-one, np.float32(-2)), 1.0, 0.0], np.float32)
    N = sr.size
    _, R, F, gs = ops.gan_d_loss(torch.from_numpy(np.concatenate([sr, sf])).to(DEV), None, N, 'hinge', 0.0)
    gs = gs.cpu().numpy()
    inv = np.float32(1) / np.float32(N)
    assert gs[:N].tolist() == [0.0, -inv, 0.0, -inv, -inv]                      # dR/ds_r = -1 iff s_r < 1
    assert gs[N:].tolist() == [0.0, inv, 0.0, inv, inv]                         # dF/ds_f = 1 iff s_f > -1
    assert R.view(-1).tolist()[0] == 0.0 and F.view(-1).tolist()[0] == 0.0


def test_unknown_kind_and_groups_are_argument_errors():
    s = torch.zeros(8, device=DEV)
    out = torch.zeros(8, device=DEV)
    lib = pg._lib.load()
    E_ARG = pg._lib.CONSTANTS['PG_E_ARG']
    p = lambda t: t.data_ptr()
    assert lib.pg_gan_d_loss(p(s), None, p(out), p(out), p(out), p(out), 2, 2, 4, 0.0, ops._stream()) == E_ARG
    assert lib.pg_gan_d_loss(p(s), None, p(out), p(out), p(out), p(out), 2, 4, 0, 0.0, ops._stream()) == E_ARG
    assert lib.pg_gan_g_loss(p(s), p(out), p(out), 2, -1, ops._stream()) == E_ARG
    assert lib.pg_r1_seed(p(s), p(s), p(out), p(out), 0, 4, 1.0, 1.0, ops._stream()) == E_ARG


@pytest.mark.parametrize('N,E', [(3, 16), (3, 48), (4, 3072), (2, 3 * 1024 * 1024), (3, 50)])
def test_r1_seed_within_derived_bounds(N, E):
    """E = 3 x 1024^2 goes past the cap of 1024 workgroups per row (grid-stride); E = 50 leaves 150 mod 4 = 2 elements to the scalar tail
    and rows that are not 16-byte aligned; one row is all zeros."""
    rs = np.random.RandomState(E % 1000 + N)
    g = rs.randn(N, E).astype(np.float32)
    g[N // 2] = 0.0
    ss = (g.astype(np.float64) ** 2).sum(1).astype(np.float32)
    gamma, inv_n = 10.0, 1.0 / N
    g_d, ss_d = torch.from_numpy(g).to(DEV), torch.from_numpy(ss).to(DEV)
    pen, u = ops.r1_seed(g_d, ss_d, gamma, inv_n)
    pen2, u2 = ops.r1_seed(g_d, ss_d, gamma, inv_n)
    wp, ep, wu, eu = ref.r1_seed(g, ss, gamma, inv_n)
    _within(pen, wp, ep, 'r1 pen N=%d E=%d' % (N, E))
    _within(u, wu, eu, 'r1 u N=%d E=%d' % (N, E))
    assert tuple(u.shape) == (N, E) and not bool(u[N // 2].any()) and float(pen[N // 2]) == 0.0
    assert torch.equal(u.view(torch.int32), u2.view(torch.int32)) and torch.equal(pen.view(torch.int32), pen2.view(torch.int32))


# ---- end to end against the oracle ---------------------------------------------------------------------------------------------------
_nets = {}


def _fixture_nets(name):
    if name not in _nets:
        meta, data = load_fixture(name)
        G, D = build_nets(meta, DEV)
        load_fixture_params(G, data, 'G')
        load_fixture_params(D, data, 'D')
        c = meta['cfg']
        cfg = go.oc.NetCfg(c['resolution'], c['num_channels'], fmap_base=c['fmap_base'], fmap_decay=c['fmap_decay'], fmap_max=c['fmap_max'],
                           latent_size=c['latent_size'])
        _nets[name] = (meta, G, D, fixture_params(data, 'G'), fixture_params(data, 'D'), cfg)
    return _nets[name]


_OBJECTIVES = [(k, p) for k in KINDS for p in ('r1', None)] + [('logistic', 'gp')]


@pytest.mark.parametrize('n', [3, 4])
@pytest.mark.parametrize('name,alpha,seed', [('tiny16c1', 1.0, 21), ('tiny16c1', 0.5, 22), ('tiny32', 1.0, 23), ('tiny32', 0.5, 24)])
@pytest.mark.parametrize('kind,penalty', _OBJECTIVES)
def test_objectives_against_float64_oracle(kind, penalty, name, alpha, seed, n):
    meta, G, D, gp, dp, cfg = _fixture_nets(name)
    depth = cfg.max_depth
    G.depth = D.depth = depth
    G.alpha = D.alpha = alpha
    weight, drift = 10.0, (0.001 if kind == 'wgan' else 0.0)
    real, z_d, z_g, mix = synthetic(seed + n, n, cfg.num_channels, cfg.resolution, cfg.latent_size)
    want = go.d_loss_and_grads(dp, gp, cfg, real, z_d, mix, depth, alpha, kind, drift, penalty, weight)
    gwant = go.g_loss_and_grads(gp, dp, cfg, z_g, depth, alpha, kind)
    if kind == 'hinge':            # a condition on the inputs, not a tolerance: no score within 1e-3 of a kink
        assert float((1 - want['s_r']).abs().min()) > 1e-3 and float((1 + want['s_f']).abs().min()) > 1e-3
    D_loss, G_loss = pg.gan_losses(kind, penalty=penalty, penalty_weight=weight)
    pg.wgan_gp_loss.enable_graphs(False)                                        # eagerly
    if penalty == 'gp':
        pg.wgan_gp_loss.set_mixing_factors(mix)
    d_cost, d_real, d_fake = D_loss(D, G, real.to(DEV), z_d.to(DEV))
    errs = dict(d_cost=rel_err(d_cost, want['d_cost']), R=rel_err(d_real, want['R']), F=rel_err(d_fake, want['F']))
    d_cost.backward()
    mine = reference_grads(D)
    assert sorted(mine) == sorted(want['grads']), 'active-parameter set differs'
    derr = {k: go.grad_err(k, mine[k], r, want['bias_terms']) for k, r in want['grads'].items()}
    g_cost = G_loss(G, D, z_g.to(DEV))
    errs['g_cost'] = rel_err(g_cost, gwant['g_cost'])
    g_cost.backward()
    mine = reference_grads(G)
    assert sorted(mine) == sorted(gwant['grads'])
    gerr = {k: rel_err(mine[k], r) for k, r in gwant['grads'].items()}
    print('%s/%s %s alpha %g n %d: losses %s, worst D gradient %.2e, worst G gradient %.2e'
          % (kind, penalty, name, alpha, n, {k: '%.1e' % v for k, v in errs.items()}, max(derr.values()), max(gerr.values())))
    assert tuple(d_real.shape) == tuple(d_fake.shape) == (n, 1)
    assert all(v < OUT_TOL for v in errs.values()), errs
    assert all(v < GRAD_TOL for v in derr.values()), max((v, k) for k, v in derr.items())
    assert all(v < GRAD_TOL for v in gerr.values()), max((v, k) for k, v in gerr.items())


# ---- the no-penalty schedule against its WGAN twin -----------------------------------------------------------------------------------
def test_plain_schedule_matches_wgan_gp_with_lambda_zero(deterministic_forward):
    """'wgan' without a penalty on the one-pass schedule against ``wgan_gp_D_loss(iwass_lambda=0)`` on the three-pass one: with lambda = 0
    the tangent seed is 0 and the two are the same mathematics.  Bounds: those of the plan-versus-eager twins of tests/test_e2e_gpu.py
    (test_plan_replay_public_api_loop: cost 1e-6; test_launch_plan_replay_matches_eager: per tensor 1e-2, whole buffer 2e-4)."""
    meta, G, D, _, _, cfg = _fixture_nets('tiny32')
    G.depth = D.depth = cfg.max_depth
    G.alpha = D.alpha = 1.0
    real, z_d, _, mix = synthetic(31, 4, 3, 32, cfg.latent_size)
    real, z_d = real.to(DEV), z_d.to(DEV)
    pg.wgan_gp_loss.enable_graphs(False)
    D_loss, _ = pg.gan_losses('wgan', penalty=None)
    c = D_loss(D, G, real, z_d)
    c[0].backward()
    mine = grads_by_name(D)
    pg.wgan_gp_loss.set_mixing_factors(mix)
    t = pg.wgan_gp_D_loss(D, G, real, z_d, iwass_lambda=0.0)
    t[0].backward()
    twin = grads_by_name(D)
    print('d_cost %.9g, twin %.9g' % (float(c[0]), float(t[0])))
    assert abs(float(c[0]) - float(t[0])) <= 1e-6 * max(1.0, abs(float(t[0])))
    assert rel_err(c[1], t[1]) <= 1e-6 and rel_err(c[2], t[2]) <= 1e-6
    assert_same_contributions(mine, twin, tol=1e-2, total=2e-4)


# ---- one path for every objective: which loss block a step launches -------------------------------------------------------------------
@pytest.mark.parametrize('case,want', [('default', ['pg_row_sumsq', 'pg_gp_seed', 'pg_d_loss', 'pg_g_loss']),
                                       ('lambda5', ['pg_row_sumsq', 'pg_gp_seed', 'pg_d_loss', 'pg_g_loss']),
                                       ('wgan5', ['pg_row_sumsq', 'pg_gp_seed', 'pg_gan_d_loss', 'pg_gan_g_loss']),
                                       ('logistic_r1', ['pg_row_sumsq', 'pg_r1_seed', 'pg_gan_d_loss', 'pg_gan_g_loss']),
                                       ('hinge_plain', ['pg_gan_d_loss', 'pg_gan_g_loss'])])
def test_each_objective_launches_the_loss_block_of_its_family(deterministic_forward, case, want):
    """The device twin of the host test of this name: the C-ABI calls of one eager D step + G step (tiny16c1, depth 2, minibatch 4)."""
    from test_gan_losses_host import FAMILY_CASES
    meta, G, D, _, _, cfg = _fixture_nets('tiny16c1')
    G.depth = D.depth = 2
    G.alpha = D.alpha = 1.0
    real, z_d, z_g, mix = synthetic(21, 4, cfg.num_channels, cfg.resolution, cfg.latent_size)
    pair, kw = FAMILY_CASES[case]
    D_loss, G_loss = pair()
    names = []

    def hook(fn, args, name):
        names.append(name)
        return fn(*args)
    pg.wgan_gp_loss.enable_graphs(False)
    pg.wgan_gp_loss.set_mixing_factors(mix)
    before, pg._lib.CALL_HOOK = pg._lib.CALL_HOOK, hook
    try:
        D_loss(D, G, real.to(DEV), z_d.to(DEV), **kw)[0].backward()
        G_loss(G, D, z_g.to(DEV)).backward()
        torch.cuda.synchronize()
    finally:
        pg._lib.CALL_HOOK = before
        pg.wgan_gp_loss.set_mixing_factors(None)
    block = ('pg_d_loss', 'pg_g_loss', 'pg_gp_seed', 'pg_gan_d_loss', 'pg_gan_g_loss', 'pg_r1_seed', 'pg_row_sumsq')
    assert [n for n in names if n in block] == want and len(names) > len(want)


# ---- launch-plan replay ---------------------------------------------------------------------------------------------------------------
def test_r1_replays_from_a_plan_of_its_own(deterministic_forward):
    """'logistic' + 'r1' from a launch plan against eager launches at identical weights: two eager warm-up steps, the recorded one, then
    three replayed ones -- every step compared at the bounds of test_plan_replay_public_api_loop (cost 1e-6, gradient buffer 2e-4 rel. L2).
    A second objective then records plans of its own beside the first one's."""
    wl = pg.wgan_gp_loss
    plans = pg.plans

    def build():
        torch.manual_seed(21)
        shape = (1, 3, 32, 32)
        kw = dict(fmap_base=512, fmap_max=64)
        G = pg.Generator(shape, latent_size=64, **kw).cuda()
        D = pg.Discriminator(shape, **kw).cuda()
        G.depth = D.depth = 3
        return G, D, pg.FusedAdam(D.parameters(), 0.001, betas=(0.0, 0.99))

    def l2(a, b):
        return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
    D_loss, G_loss = pg.gan_losses('logistic', penalty='r1', penalty_weight=10.0)
    wl.enable_graphs(False)                                                     # (drops whatever earlier tests recorded)
    plans.STATS.update(recorded=0, replayed=0)
    gen = torch.Generator(device='cuda').manual_seed(9)
    wl.manual_seed(5)
    try:
        (Ga, Da, oa), (Gb, Db, ob) = build(), build()
        for it in range(6):
            real = torch.rand((6, 3, 32, 32), device=DEV, generator=gen) * 2 - 1
            z = torch.randn((6, 64), device=DEV, generator=gen)
            zg = torch.randn((6, 64), device=DEV, generator=gen)
            out = []
            for (G, D, opt), mode in (((Ga, Da, oa), 'auto'), ((Gb, Db, ob), False)):
                wl._use_graphs = mode                                           # (the switch itself: enable_graphs(False) would drop the recorded plans)
                c = D_loss(D, G, real, z)[0]
                c.backward()
                dg = D._flat_grad.clone()
                g = G_loss(G, D, zg)
                g.backward()
                out.append((float(c), dg, float(g), G._flat_grad.clone()))
                opt.step()
            torch.cuda.synchronize()
            (ca, dga, ga, gga), (cb, dgb, gb, ggb) = out
            print('step %d: d_cost %.9g | %.9g, g_cost %.9g | %.9g, D gradients %.2e, G gradients %.2e' % (it, ca, cb, ga, gb, l2(dga, dgb), l2(gga, ggb)))
            assert abs(ca - cb) <= 1e-6 * max(1.0, abs(cb)) and abs(ga - gb) <= 1e-6 * max(1.0, abs(gb)), it
            assert l2(dga, dgb) < 2e-4 and l2(gga, ggb) < 2e-4, it
            with torch.no_grad():                                               # keep the twins at identical weights / moments
                Db._flat_param.copy_(Da._flat_param)
            Db.mark_params_changed()
            for (_, ma, va), (_, mb_, vb) in zip(oa._flat.values(), ob._flat.values()):
                mb_.copy_(ma)
                vb.copy_(va)
        assert plans.STATS['recorded'] == 2 and plans.STATS['replayed'] == 2 * 3, plans.STATS
        assert wl._seed[1] == 0                                                 # R1 draws no mixing factors
        keys = list(plans._CACHE)
        obj = D_loss.objective
        assert sorted(k[0][0] for k in keys) == ['D', 'G'] and all(k[1][-1] == obj for k in keys)      # (stage part, variant part)
        # a second objective in the same process: plans of its own, beside the first one's
        wl._use_graphs = 'auto'
        D2, G2 = pg.gan_losses('hinge', penalty='r1', penalty_weight=1.0)
        for _ in range(3):
            D2(Da, Ga, real, z)[0].backward()
            G2(Ga, Da, zg).backward()
        torch.cuda.synchronize()
        assert plans.STATS['recorded'] == 4
        by_obj = {}
        for k, plan in plans._CACHE.items():
            by_obj.setdefault(k[1][-1], []).append(plan)
        assert set(by_obj) == {obj, D2.objective} and all(len(v) == 2 and all(p.entries is not None for p in v) for v in by_obj.values())
        assert len({id(p) for v in by_obj.values() for p in v}) == 4
        # ... and WGAN-GP's own key ends in its objective on the original kernels
        pg.wgan_gp_D_loss(Da, Ga, real, z)[0].backward()
        assert sum(1 for k in plans._CACHE if k[0][0] == 'D' and k[1][-1] is pg.engine.WGAN_GP) == 1
    finally:
        wl.enable_graphs(False)


# ---- Trainer --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,penalty', [('logistic', 'r1'), ('hinge', None)])
def test_trainer_iterations(kind, penalty):
    wl = pg.wgan_gp_loss
    meta, data = load_fixture('tiny32')
    G, D = build_nets(meta, DEV)
    load_fixture_params(G, data, 'G')
    load_fixture_params(D, data, 'D')
    G.depth = D.depth = 3
    c = meta['cfg']
    if kind == 'hinge':
        # With every score inside the margins the hinge terms are linear and d cost / d linear.bias = N (-1/N) + N (1/N) is exactly zero:
        # Adam would rightly leave that one tensor alone.  Start from scores that straddle the real side's margin instead.
        with torch.no_grad():
            D.linear.bias.fill_(1.0)
        D.mark_params_changed()
    opt_g = pg.FusedAdam(G.parameters(), 0.001, betas=(0.0, 0.99))
    opt_d = pg.FusedAdam(D.parameters(), 0.001, betas=(0.0, 0.99))
    ds = pg.utils.SyntheticDataset(32, 3, seed=5)
    ds.model_depth = 3
    D_loss, G_loss = pg.gan_losses(kind, penalty=penalty, penalty_weight=10.0)
    tr = pg.Trainer(D, G, D_loss, G_loss, opt_d, opt_g, ds, ds.loader(4), pg.utils.device_latents(4, c['latent_size'], seed=3))
    losses = []

    class Rec(pg.Plugin):
        def __init__(self):
            super(Rec, self).__init__([(1, 'iteration')])

        def register(self, trainer):
            pass

        def iteration(self, i, g_cost, d_cost, d_real, d_fake):
            losses.append([float(g_cost), float(d_cost)] + d_real.view(-1).tolist() + d_fake.view(-1).tolist())
    tr.register_plugin(Rec())
    before = {k: v.detach().clone() for net in (G, D) for k, v in ((id(p), p) for p in net.parameters())}
    wl.enable_graphs('auto')
    wl.manual_seed(123)
    try:
        for _ in range(3):
            tr.train()
        torch.cuda.synchronize()
        assert wl._seed == [123, 0, None]                                       # the mixing-factor stream was not touched
        assert len(losses) == 3 and all(len(row) == 2 + 8 and np.all(np.isfinite(row)) for row in losses), losses
        params = [p for net in (G, D) for p in net.parameters()]
        active = [p for p in params if p.grad is not None]
        # fully grown at alpha 1: everything but the toRGB / fromRGB layers of the coarser stages (3 per network, weight and bias)
        assert len(active) == len(params) - 2 * 3 * 2, (len(active), len(params))
        assert all(bool((p.detach() != before[id(p)]).any()) for p in active)
        assert all(torch.equal(p.detach(), before[id(p)]) for p in params if p.grad is None)
    finally:
        wl.enable_graphs(False)
