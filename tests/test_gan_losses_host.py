"""Selectable GAN objectives, CPU tier: the fp64 references of tests/gan_losses_ref.py against float64 autograd of
the table's expressions; the engine's schedules for every kind x {'gp', 'r1', None} on the CPU emulation of the kernels
(tests/emu_ops.py + tests/emu_gan_losses.py) against float64 autograd through the oracle's networks; the public interface; the header."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import emu_gan_losses
import emu_ops
import gan_losses_oracle as go
import gan_losses_ref as ref
from conftest import ROOT, fixture_params, load_fixture, rel_err
from helpers import build_nets, load_fixture_params, reference_grads, synthetic
from test_engine_host import GRAD_TOL, OUT_TOL      # the bounds test_schedules_match_reference applies to WGAN-GP on the same fixtures

import pggan_amd as pg

KINDS = ref.KINDS
PENALTIES = ('gp', 'r1', None)


@pytest.fixture()
def emu(monkeypatch):
    for name in ('gan_d_loss', 'gan_g_loss', 'r1_seed'):
        monkeypatch.setattr(emu_ops, name, getattr(emu_gan_losses, name), raising=False)
    for modname in ('engine', 'optim'):
        monkeypatch.setattr(importlib.import_module('pggan-pytorch_amd.' + modname), 'ops', emu_ops)
    monkeypatch.setattr(pg.engine, '_check_dev', lambda t, what: t.contiguous())
    yield


# ---- the references against float64 autograd -----------------------------------------------------------------------------------------
def _scores(n, seed):
    rs = np.random.RandomState(seed)
    s = (rs.randn(n) * 3).astype(np.float32)
    k = min(n, ref.FIXED_SCORES.size)
    s[:k] = ref.FIXED_SCORES[:k]
    return s


def _close(a, b, what):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b))), (what, np.abs(a - b).max())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('groups,with_pen', [(2, False), (3, True), (3, False)])
def test_loss_references_match_float64_autograd(kind, groups, with_pen):
    N, drift = 40, 0.125
    s32 = np.concatenate([_scores(N, 1), _scores(N, 2)[::-1], np.zeros((groups - 2) * N, np.float32)])
    assert np.any(s32[:N] == 1.0) and np.any(s32[N:2 * N] == -1.0)              # the kinks of the hinge terms are among the scores
    pen = np.random.RandomState(3).rand(N).astype(np.float32) if with_pen else None
    out = ref.gan_d_loss(s32, pen, N, groups, kind, drift)
    s = torch.tensor(s32, dtype=torch.float64, requires_grad=True)
    R = go.real_term(kind, s[:N]) + drift * s[:N] ** 2
    F = go.fake_term(kind, s[N:2 * N])
    cost = (F + R + (torch.tensor(pen, dtype=torch.float64) if with_pen else 0)).mean()
    gs, = torch.autograd.grad(cost, s)
    _close(out['d_cost'][0], cost.item(), 'd_cost')
    _close(out['d_real'][0], R.detach().numpy(), 'R')
    _close(out['d_fake'][0], F.detach().numpy(), 'F')
    _close(out['gscore'][0], gs.numpy(), 'gscore')
    assert out['gscore'][0].shape == (groups * N,) and all(np.all(b >= 0) for _, b in out.values())
    if kind == 'hinge':                                                          # exactly 0 at the kink: torch's relu subgradient
        assert np.all(out['gscore'][0][:N][s32[:N] == 1.0] == 2 * drift / N) and np.all(out['gscore'][0][N:2 * N][s32[N:2 * N] == -1.0] == 0.0)
    sg = torch.tensor(s32[:N], dtype=torch.float64, requires_grad=True)
    g_cost = go.generator_term(kind, sg).mean()
    gg, = torch.autograd.grad(g_cost, sg)
    c, _, gscore, _ = ref.gan_g_loss(s32[:N], kind)
    _close(c, g_cost.item(), 'g_cost')
    _close(gscore, gg.numpy(), 'g gscore')


def test_r1_reference_matches_float64_autograd():
    N, E, gamma = 4, 50, 10.0
    g32 = np.random.RandomState(5).randn(N, E).astype(np.float32)
    g32[2] = 0.0
    ss = (g32.astype(np.float64) ** 2).sum(1)
    pen, _, u, _ = ref.r1_seed(g32, ss, gamma, 1.0 / N)
    g = torch.tensor(g32, dtype=torch.float64, requires_grad=True)
    p = 0.5 * gamma * (g ** 2).sum(1)
    du, = torch.autograd.grad(p.mean(), g)
    _close(pen, p.detach().numpy(), 'pen')
    _close(u, du.numpy(), 'u')
    assert np.all(u[2] == 0.0) and pen[2] == 0.0


def test_emulation_agrees_with_the_references():
    """tests/emu_gan_losses.py (what the engine runs on in this tier) states the same functions as tests/gan_losses_ref.py."""
    N = 24
    s32 = np.concatenate([_scores(N, 7), _scores(N, 8), np.zeros(N, np.float32)])
    pen = np.random.RandomState(9).rand(N).astype(np.float32)
    for kind in KINDS:
        want = ref.gan_d_loss(s32, pen, N, 3, kind, 0.125)                  # (a drift that fp32 holds exactly: the reference rounds it as the C ABI does)
        got = emu_gan_losses.gan_d_loss(torch.tensor(s32, dtype=torch.float64), torch.tensor(pen, dtype=torch.float64), N, kind, 0.125)
        for a, name in zip(got, ('d_cost', 'd_real', 'd_fake', 'gscore')):
            _close(a.numpy(), want[name][0], (kind, name))
        c, _, gs, _ = ref.gan_g_loss(s32[:N], kind)
        gc, ggs = emu_gan_losses.gan_g_loss(torch.tensor(s32[:N], dtype=torch.float64), kind)
        _close(gc.numpy(), c, kind)
        _close(ggs.numpy(), gs, kind)


# ---- the engine on the CPU emulation against the oracle ------------------------------------------------------------------------------
_STAGES = [('tiny16c1', 1.0, 21), ('tiny16c1', 0.5, 22), ('tiny32', 1.0, 23), ('tiny32', 0.5, 24)]
_nets = {}


def _fixture_nets(name):
    if name not in _nets:
        meta, data = load_fixture(name)
        G, D = build_nets(meta)
        load_fixture_params(G, data, 'G')
        load_fixture_params(D, data, 'D')
        c = meta['cfg']
        cfg = go.oc.NetCfg(c['resolution'], c['num_channels'], fmap_base=c['fmap_base'], fmap_decay=c['fmap_decay'], fmap_max=c['fmap_max'],
                           latent_size=c['latent_size'])
        _nets[name] = (meta, G, D, fixture_params(data, 'G'), fixture_params(data, 'D'), cfg)
    return _nets[name]


@pytest.mark.parametrize('name,alpha,seed', _STAGES)
@pytest.mark.parametrize('penalty', PENALTIES)
@pytest.mark.parametrize('kind', KINDS)
def test_engine_matches_float64_oracle(emu, kind, penalty, name, alpha, seed):
    """Minibatch 4.  The draws (``_STAGES``) are ones on which the fp32 emulation and the fp64 oracle take the same LeakyReLU branches: a
    pre-activation within fp32 round-off of zero moves fromRGB's gradient by 1e-3 .. 6e-3 for EVERY objective, WGAN-GP included (seed 27 on
    tiny32 does), which is the networks' property (tests/test_e2e_gpu.py, header), not the loss block's."""
    meta, G, D, gp, dp, cfg = _fixture_nets(name)
    depth = cfg.max_depth
    G.depth = D.depth = depth
    G.alpha = D.alpha = alpha
    n, weight, drift = 4, 10.0, (0.001 if kind == 'wgan' else 0.0)
    real, z_d, z_g, mix = synthetic(seed, n, cfg.num_channels, cfg.resolution, cfg.latent_size)
    D_loss, G_loss = pg.gan_losses(kind, penalty=penalty, penalty_weight=weight)
    want = go.d_loss_and_grads(dp, gp, cfg, real, z_d, mix, depth, alpha, kind, drift, penalty, weight)
    gwant = go.g_loss_and_grads(gp, dp, cfg, z_g, depth, alpha, kind)
    if kind == 'hinge':            # a condition on the inputs, not a tolerance: no score within 1e-3 of a kink
        assert float((1 - want['s_r']).abs().min()) > 1e-3 and float((1 + want['s_f']).abs().min()) > 1e-3
    pg.wgan_gp_loss.manual_seed(77)
    counter = pg.wgan_gp_loss._seed[1]
    if penalty == 'gp':
        pg.wgan_gp_loss.set_mixing_factors(mix)
    d_cost, d_real, d_fake = D_loss(D, G, real, z_d)
    assert pg.wgan_gp_loss._seed[1] == counter and pg.wgan_gp_loss.mixing_factors is None     # injected or not needed: nothing drawn
    assert tuple(d_real.shape) == tuple(d_fake.shape) == (n, 1) and d_cost.dim() == 0
    assert rel_err(d_cost, want['d_cost']) < OUT_TOL
    assert rel_err(d_real, want['R']) < OUT_TOL and rel_err(d_fake, want['F']) < OUT_TOL
    d_cost.backward()
    mine = reference_grads(D)
    assert sorted(mine) == sorted(want['grads']), 'active-parameter set differs'
    for k, r in want['grads'].items():
        assert go.grad_err(k, mine[k], r, want['bias_terms']) < GRAD_TOL, (k, go.grad_err(k, mine[k], r, want['bias_terms']))
    assert all(p.grad is None for p in G.parameters())
    g_cost = G_loss(G, D, z_g)
    assert rel_err(g_cost, gwant['g_cost']) < OUT_TOL
    g_cost.backward()
    mine = reference_grads(G)
    assert sorted(mine) == sorted(gwant['grads'])
    for k, r in gwant['grads'].items():
        assert rel_err(mine[k], r) < GRAD_TOL, (k, rel_err(mine[k], r))


def test_backward_scale_and_return_all(emu):
    """``d_cost.backward(gradient)`` of the no-penalty schedule rescales the gradients; ``return_all=False`` returns the cost alone."""
    meta, G, D, gp, dp, cfg = _fixture_nets('tiny16c1')
    G.depth = D.depth = 2
    G.alpha = D.alpha = 1.0
    real, z_d, _, _ = synthetic(3, 4, 1, 16, cfg.latent_size)
    D_loss, _ = pg.gan_losses('hinge', penalty=None)
    D_loss(D, G, real, z_d)[0].backward()
    base = D._flat_grad.clone()
    c = D_loss(D, G, real, z_d, return_all=False)
    assert torch.is_tensor(c) and c.dim() == 0
    c.backward(torch.tensor(0.5))
    assert float(base.abs().max()) > 0 and torch.allclose(D._flat_grad, 0.5 * base, rtol=1e-6, atol=0)


# ---- one path for every objective: which loss block a step launches -------------------------------------------------------------------
LOSS_BLOCK = ('d_loss', 'g_loss', 'gp_seed', 'gan_d_loss', 'gan_g_loss', 'r1_seed', 'row_sumsq')
FAMILY_CASES = {                # name -> (the pair, keyword arguments of its D loss)
    'default': (lambda: (pg.wgan_gp_D_loss, pg.wgan_gp_G_loss), {}),
    'lambda5': (lambda: (pg.wgan_gp_D_loss, pg.wgan_gp_G_loss), dict(iwass_lambda=5.0)),
    'wgan5': (lambda: pg.gan_losses('wgan', penalty_weight=5.0), {}),
    'logistic_r1': (lambda: pg.gan_losses('logistic', penalty='r1'), {}),
    'hinge_plain': (lambda: pg.gan_losses('hinge', penalty=None), {}),
}


class _Recording(object):
    """Stands in for ``engine.ops``: the emulation, with the name and the arguments of every function call kept in ``calls``."""

    def __init__(self, mod):
        self._mod, self.calls = mod, []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not callable(fn) or isinstance(fn, type):
            return fn

        def recorded(*a, **k):
            self.calls.append((name, a, k))
            return fn(*a, **k)
        return recorded


def _recorded_step(case, monkeypatch):
    meta, G, D, gp, dp, cfg = _fixture_nets('tiny16c1')
    G.depth = D.depth = 2
    G.alpha = D.alpha = 1.0
    real, z_d, z_g, mix = synthetic(21, 4, cfg.num_channels, cfg.resolution, cfg.latent_size)
    pair, kw = FAMILY_CASES[case]
    D_loss, G_loss = pair()
    rec = _Recording(pg.engine.ops)
    monkeypatch.setattr(pg.engine, 'ops', rec)
    pg.wgan_gp_loss.set_mixing_factors(mix)
    try:
        d_cost = D_loss(D, G, real, z_d, **kw)[0]
        d_cost.backward()
        d_grad = D._flat_grad.clone()
        G_loss(G, D, z_g).backward()
    finally:
        pg.wgan_gp_loss.set_mixing_factors(None)         # ('r1' and no penalty leave it where it is)
    return [c for c in rec.calls if c[0] in LOSS_BLOCK], float(d_cost), d_grad


@pytest.mark.parametrize('case,want', [('default', ['row_sumsq', 'gp_seed', 'd_loss', 'g_loss']),
                                       ('lambda5', ['row_sumsq', 'gp_seed', 'd_loss', 'g_loss']),
                                       ('wgan5', ['row_sumsq', 'gp_seed', 'gan_d_loss', 'gan_g_loss']),
                                       ('logistic_r1', ['row_sumsq', 'r1_seed', 'gan_d_loss', 'gan_g_loss']),
                                       ('hinge_plain', ['gan_d_loss', 'gan_g_loss'])])
def test_each_objective_launches_the_loss_block_of_its_family(emu, monkeypatch, case, want):
    """One D step + G step on the emulation: the default pair and ``wgan_gp_D_loss`` with another lambda stay on the original loss block
    (no ``gan_*`` / ``r1_seed``), every ``gan_losses`` closure on the pinned one; without a penalty there is no seed and no ``row_sumsq``
    and the loss block is handed ``pen=None``."""
    calls, _, _ = _recorded_step(case, monkeypatch)
    assert [c[0] for c in calls] == want
    if case == 'hinge_plain':
        name, a, k = calls[0]
        assert (a[1] if len(a) > 1 else k['pen']) is None
    if case in ('lambda5', 'wgan5'):
        assert [c[1][2] for c in calls if c[0] == 'gp_seed'] == [5.0]


def test_the_two_families_state_the_same_wgan_gp(emu, monkeypatch):
    """``wgan_gp_D_loss(iwass_lambda=5)`` (original block) against ``gan_losses('wgan', penalty_weight=5)`` (pinned block): the same formula
    over 4 scores, which the emulation evaluates in float64 -- equal up to the final cast, held to 1e-5 relative."""
    _, cost_o, grad_o = _recorded_step('lambda5', monkeypatch)
    _, cost_p, grad_p = _recorded_step('wgan5', monkeypatch)
    assert abs(cost_o - cost_p) <= 1e-5 * abs(cost_o)
    assert float(grad_o.abs().max()) > 0 and rel_err(grad_p, grad_o) <= 1e-5


def test_plan_keys_split_into_stage_and_variants(monkeypatch):
    """Two objectives, and two ``iwass_lambda`` values, at one stage differ in the variant part of the plan key only and live side by side;
    a stage change of the same network pair drops both.  (The key function and the cache alone: no plan is recorded.)"""
    plans, eng = pg.plans, pg.engine
    meta, G, D, gp, dp, cfg = _fixture_nets('tiny16c1')
    monkeypatch.setattr(plans, '_CACHE', type(plans._CACHE)())
    objs = [eng.WGAN_GP, eng.WGAN_GP._replace(weight=5.0), pg.gan_losses('logistic', penalty='r1')[0].objective]

    def key(depth, obj):
        return plans._key('D', D, G, (depth, (4, 1, 16, 16), (4, cfg.latent_size)), ((0, None), 0, obj))
    keys = [key(2, o) for o in objs]
    assert len(set(keys)) == 3 and len({k[0] for k in keys}) == 1 and [k[1][-1] for k in keys] == objs
    for k in keys:
        plans._new_plan(k)
    g_key = plans._key('G', D, G, (2, (4, cfg.latent_size), (0, None), False), (objs[0],))
    plans._new_plan(g_key)                               # (MAX_PLANS = 4: the three D variants and a G plan)
    assert list(plans._CACHE) == keys + [g_key]
    moved = key(1, objs[1])
    assert moved[0] != keys[0][0] and moved[1] == keys[1][1]
    plans._new_plan(moved)
    assert list(plans._CACHE) == [g_key, moved]          # every D variant of the stage it left is gone; the G plans are another step's


# ---- the public interface -------------------------------------------------------------------------------------------------------------
def test_default_objective_is_the_existing_pair():
    assert pg.gan_losses('wgan', penalty='gp') == (pg.wgan_gp_D_loss, pg.wgan_gp_G_loss)
    d, g = pg.gan_losses()
    assert d is pg.wgan_gp_D_loss and g is pg.wgan_gp_G_loss
    d, g = pg.gan_losses('wgan', penalty='gp', penalty_weight=10.0, drift=0.001, gp_target=1.0)
    assert d is pg.wgan_gp_D_loss and g is pg.wgan_gp_G_loss
    for kw in (dict(penalty_weight=5.0), dict(drift=0.0), dict(gp_target=750.0), dict(penalty='r1'), dict(penalty=None)):
        d, g = pg.gan_losses('wgan', **dict(dict(penalty='gp'), **kw))
        assert d is not pg.wgan_gp_D_loss and g is not pg.wgan_gp_G_loss and d.objective == g.objective
    d, _ = pg.gan_losses('logistic', penalty='r1', penalty_weight=10.0)
    assert d.objective == pg.engine.Objective('logistic', 0.0, 'r1', 10.0, 1.0) and hash(d.objective) == hash(tuple(d.objective))
    with pytest.raises(AttributeError):
        d.objective.kind = 'wgan'                                                # immutable: it is part of a plan's key


@pytest.mark.parametrize('args,kw', [(('wasserstein',), {}), (('logistic',), dict(penalty='r2')), (('logistic',), dict(penalty='R1')),
                                     (('hinge',), dict(penalty_weight=0.0)), (('hinge',), dict(penalty_weight=-1.0)),
                                     (('lsgan',), dict(penalty='r1', penalty_weight=float('nan'))), (('wgan',), dict(gp_target=0.0)),
                                     (('wgan',), dict(drift=-0.1)), ((None,), {})])
def test_bad_arguments_raise_value_error(args, kw):
    with pytest.raises(ValueError):
        pg.gan_losses(*args, **kw)


# ---- the header -----------------------------------------------------------------------------------------------------------------------
def test_gan_header_parses_completely():
    """Every prototype of include/pggan_hip_gan.h lands in _lib.GAN_SIGNATURES and every #define in GAN_CONSTANTS; the product header's
    tables are not touched by the addition; the kind numbers in ops.py are the header's."""
    _lib = pg._lib
    with open(os.path.join(ROOT, 'include', 'pggan_hip_gan.h')) as f:
        text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', f.read(), flags=re.S)
    protos = re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', text)
    assert sorted(protos) == sorted(_lib.GAN_SIGNATURES) == ['pg_gan_d_loss', 'pg_gan_g_loss', 'pg_r1_seed']
    defines = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(PG_\w+)[ \t]+(\S+)[ \t]*$', text, flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == _lib.GAN_CONSTANTS == dict(PG_GAN_WGAN=0, PG_GAN_LOGISTIC=1, PG_GAN_HINGE=2, PG_GAN_LSGAN=3)
    P, I, L, F = _lib.P, _lib.I, _lib.L, _lib.F
    assert _lib.GAN_SIGNATURES['pg_gan_d_loss'] == [P, P, P, P, P, P, I, I, I, F, P]
    assert _lib.GAN_SIGNATURES['pg_gan_g_loss'] == [P, P, P, I, I, P]
    assert _lib.GAN_SIGNATURES['pg_r1_seed'] == [P, P, P, P, I, L, F, F, P]
    assert not set(_lib.GAN_SIGNATURES) & set(_lib.SIGNATURES) and not set(_lib.GAN_CONSTANTS) & set(_lib.CONSTANTS)
    assert pg.ops.GAN_KINDS == dict(wgan=0, logistic=1, hinge=2, lsgan=3) and tuple(pg.ops.GAN_KINDS) == KINDS
    src = open(os.path.join(ROOT, 'pggan-pytorch_amd', 'ops.py')).read() + open(os.path.join(ROOT, 'pggan-pytorch_amd', 'gan_losses.py')).read()
    assert not re.search(r"'(?:wgan|logistic|hinge|lsgan)'\s*:\s*\d", src)      # mirrored from the header, never retyped
