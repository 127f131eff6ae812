"""Host tier of the differentiable augmentation (pggan-pytorch_amd/augment.py, plugins.AugmentController, gan_losses(augment=...)): the
numpy twin against the literal loop nest of tests/augment_ref.py with ``==``, transposition, the table twin, the controller's rule on a
stub accumulator, and the step hooks of ``engine`` on the CPU emulation of the kernels against float64 autograd.  No GPU, no library."""
import importlib
import itertools

import numpy as np
import pytest
import torch

import augment_ref as ar
import emu_gan_losses
import emu_ops
from conftest import fixture_params, load_fixture, rel_err
from helpers import build_nets, load_fixture_params, reference_grads, synthetic

import pggan_amd as pg

A = pg.augment


def _cutouts(H, W):
    """empty, one pixel, full width, full height, everything"""
    return [(0, 0, 0, 0), (1, 2, W - 1, W), (H - 1, H, 0, W), (0, H, 0, 1), (0, H, 0, W)]


@pytest.mark.parametrize('shape', [(2, 2, 4, 4), (3, 1, 8, 8)])
def test_twin_is_the_loop_nest(shape):
    """Every combination of flip, dx in -W .. W, dy in {0, +-1, +-H} and an empty, one-pixel, full-width, full-height or full cutout, with and
    without a gain: forward and transpose of the twin equal the loop nest bit for bit."""
    N, C, H, W = shape
    x = ar.images(N, C, H, W, seed=11)
    g = ar.images(N, C, H, W, seed=12)
    rows = [ar.row(flip, dy, dx, *cut, gain=gain)
            for flip, dx, dy, cut in itertools.product((0, 1), range(-W, W + 1), (0, 1, -1, H, -H), _cutouts(H, W))
            for gain in ((None, 0.5) if (dx + dy) % 4 == 0 else (None,))]
    rows += [rows[k] for k in range(-len(rows) % N)]
    assert len(rows) >= 2 * (2 * W + 1) * 5 * 5
    for k in range(0, len(rows), N):
        table = np.asarray(rows[k:k + N], dtype=np.int32)
        mask = 1 if (k // N) % 2 else (1 << C) - 1                               # channel 0 only / every channel
        assert np.array_equal(ar.bits(A.apply_host(x, table, mask)), ar.bits(ar.apply_loops(x, table, mask))), table
        assert np.array_equal(ar.bits(A.adjoint_host(g, table)), ar.bits(ar.adjoint_loops(g, table))), table


def test_identity_row_copies_bits_and_padding_is_plus_zero():
    x = ar.images(2, 2, 4, 4, seed=3)
    assert np.signbit(x).any() and (x == 0).any()
    ident = np.zeros((2, 8), dtype=np.int32)
    assert np.array_equal(ar.bits(A.apply_host(x, ident)), ar.bits(x))
    assert np.array_equal(ar.bits(A.adjoint_host(A.apply_host(x, ident), ident)), ar.bits(x))
    gone = np.asarray([ar.row(dy=4), ar.row(y0=0, y1=4, x0=0, x1=4)], dtype=np.int32)       # shifted out / cut out: +0.0 everywhere
    assert not ar.bits(A.apply_host(-np.abs(x) - 1, gone)).any() and not ar.bits(A.adjoint_host(-np.abs(x) - 1, gone)).any()
    # a gain row adds to the source pixels only: the padding and the cutout stay +0.0
    y = A.apply_host(x, np.asarray([ar.row(dx=1, gain=0.5), ar.row(y0=1, y1=3, x0=0, x1=4, gain=0.5)], dtype=np.int32), 1)
    assert not ar.bits(y[0, :, :, 0]).any() and not ar.bits(y[1, :, 1:3]).any()
    assert np.array_equal(y[0, 0, :, 1:], (x[0, 0, :, :3] + np.float32(0.5)).astype(np.float32)) and np.array_equal(ar.bits(y[0, 1, :, 1:]), ar.bits(x[0, 1, :, :3]))


@pytest.mark.parametrize('shape', [(2, 2, 4, 4), (3, 1, 8, 8)])
def test_adjoint_is_the_transpose(shape):
    """<apply(x), g> == <x, adjoint(g)> exactly: small integers, no gain (every product and every partial sum is an integer below 2^24)."""
    N, C, H, W = shape
    rs = np.random.RandomState(5)
    x = rs.randint(-8, 9, size=shape).astype(np.float32)
    g = rs.randint(-8, 9, size=shape).astype(np.float32)
    pool = ar.pool(H, W, gain=False)
    for k in range(0, len(pool) - N + 1, N):
        table = pool[k:k + N]
        lhs = (A.apply_host(x, table).astype(np.float64) * g).sum()
        rhs = (x.astype(np.float64) * A.adjoint_host(g, table)).sum()
        assert lhs == rhs, table


# ------------------------------------------------------------------------------------------ tables
def test_uniform_twin_is_philox():
    from philox_ref import _philox4x32_10
    seed, draw = 0x123456789abcdef, 5
    u = A.uniform_host(seed, draw, 11)
    want = []
    for e in range(11):
        c = _philox4x32_10([e // 4, 0, draw, 0], [seed & 0xffffffff, seed >> 32])
        want.append(np.float32(c[e % 4] >> 8) * np.float32(1.0 / 16777216.0))
    assert u.dtype == np.float32 and u.tolist() == [float(w) for w in want]


POLICY = dict(translate=(0.25, 0.125), cutout=(0.5, 0.25), gain=0.5, gain_channels=(0,), flip=True)


def test_table_twin_properties():
    H, W, rows = 16, 64, 400
    none = pg.Augmenter(p=0.0, device='cpu', **POLICY).table(rows, H, W, 'd')
    assert none.dtype == torch.int32 and tuple(none.shape) == (rows, 8) and not none.any()      # p = 0: identity rows
    t = pg.Augmenter(p=1.0, seed=7, device='cpu', **POLICY).table(rows, H, W, 'd').numpy()
    flags, dy, dx, y0, y1, x0, x1 = (t[:, k] for k in range(7))
    b = t[:, 7].copy().view(np.float32)
    assert (flags & 2).all() and 0.3 < (flags & 1).mean() < 0.7                                 # p = 1: every operation (the flip: a coin)
    assert np.abs(dy).max() == 4 and np.abs(dx).max() == 8                                      # floor(ry H), floor(rx W): reached, never passed
    assert set(dy.tolist()) == set(range(-4, 5)) and set(dx.tolist()) == set(range(-8, 9))
    assert (0 <= y0).all() and (y0 < y1).all() and (y1 <= H).all() and (0 <= x0).all() and (x0 < x1).all() and (x1 <= W).all()
    assert (y1 - y0).max() == 8 and (x1 - x0).max() == 16 and (y1 - y0).min() >= 4 and (x1 - x0).min() >= 8      # round(ch H) x round(cw W), clipped at the edges
    assert (np.abs(b) <= 0.5).all() and b.min() < -0.3 and b.max() > 0.3 and len(set(b.tolist())) > rows // 2
    # ratio 1.0 on an axis: the whole axis (a full-height time mask)
    m = pg.Augmenter(p=1.0, translate=(0, 0), cutout=(1.0, 0.125), device='cpu').table(50, H, W, 'g').numpy()
    assert (m[:, 3] == 0).all() and (m[:, 4] == H).all() and ((m[:, 6] - m[:, 5]) <= 8).all() and not m[:, [0, 1, 2, 7]].any()
    # 0 < p < 1: each operation about p of the rows, independently
    h = pg.Augmenter(p=0.5, seed=3, device='cpu', **POLICY).table(2000, H, W, 'd').numpy()
    on = np.stack([(h[:, 0] & 2) != 0, h[:, 4] > h[:, 3], (h[:, 1] != 0) | (h[:, 2] != 0)])
    assert (np.abs(on.mean(axis=1) - [0.5, 0.5, 0.5 * (1 - 1 / (9 * 17))]) < 0.05).all()
    assert abs(((h[:, 0] & 1) != 0).mean() - 0.25) < 0.04
    assert np.abs(np.corrcoef(on.astype(np.float64))[np.triu_indices(3, 1)]).max() < 0.08


def test_tables_are_a_function_of_seed_and_counter():
    a, b = pg.Augmenter(seed=9, device='cpu', **POLICY), pg.Augmenter(seed=9, device='cpu', **POLICY)
    d0, g0, d1 = a.table(6, 16, 16, 'd'), a.table(3, 16, 16, 'g'), a.table(6, 16, 16, 'd')
    # the other order of D and G steps: the same tables per stream
    e0, e1, h0 = b.table(6, 16, 16, 'd'), b.table(6, 16, 16, 'd'), b.table(3, 16, 16, 'g')
    assert torch.equal(d0, e0) and torch.equal(d1, e1) and torch.equal(g0, h0)
    assert not torch.equal(d0, d1) and not torch.equal(d0[:3], g0) and a.draws == {'d': 2, 'g': 1}
    assert not torch.equal(pg.Augmenter(seed=10, device='cpu', **POLICY).table(6, 16, 16, 'd'), d0)
    # the uniforms behind them: draw numbers 2 k for 'd', 2 k + 1 for 'g'
    U = A.uniform_host(9, 2, 48).reshape(6, 8)
    assert np.array_equal(A.table_host(U, 16, 16, 0.25, 0.125, 0.5, 0.25, 0.5, True, 1.0), d1.numpy())
    # an injected table is handed out once, draws nothing, and the next call draws again
    mine = np.arange(24, dtype=np.int32).reshape(3, 8)
    a.inject(g_table=mine)
    assert np.array_equal(a.next_table('g', 3, 16, 16).numpy(), mine) and a.draws == {'d': 2, 'g': 1}
    assert torch.equal(a.next_table('g', 3, 16, 16), b.table(3, 16, 16, 'g'))
    a.inject(d_table=mine)
    with pytest.raises(ValueError):
        a.next_table('d', 6, 16, 16)


def test_constants_are_the_header_s():
    C = pg._lib.AUGMENT_CONSTANTS
    assert (A.COLS, A.FLIP, A.GAIN, A.MAX_SIZE) == (C['PG_AUGMENT_COLS'], C['PG_AUGMENT_FLIP'], C['PG_AUGMENT_GAIN'], C['PG_AUGMENT_MAX_SIZE'])
    assert (ar.FLIP, ar.GAIN) == (A.FLIP, A.GAIN)
    assert set(pg._lib.AUGMENT_SIGNATURES) == {'pg_augment_apply', 'pg_augment_adjoint', 'pg_augment_table', 'pg_score_signs'}
    assert not set(pg._lib.AUGMENT_SIGNATURES) & set(pg._lib.SIGNATURES)


# ------------------------------------------------------------------------------------------ arguments
@pytest.mark.parametrize('kw', [dict(p=-0.1), dict(p=1.5), dict(translate=(0.0, 1.5)), dict(translate=(-0.1, 0.0)), dict(cutout=(2.0, 0.0)),
                                dict(cutout=(0.0, -1.0)), dict(gain=-0.5), dict(gain=float('nan')), dict(p=float('nan')), dict(gain_channels=(32,))])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        pg.Augmenter(device='cpu', **kw)


def test_controller_refuses():
    aug = pg.Augmenter(device='cpu')
    for kw in (dict(target=1.0), dict(target=-1.5), dict(adjust_kimg=0), dict(adjust_kimg=-1), dict(interval=0), dict(interval=1.5),
               dict(p_max=1.5), dict(p_max=-0.1)):
        with pytest.raises(ValueError):
            pg.AugmentController(aug, **kw)
    with pytest.raises(ValueError):
        pg.AugmentController(object())
    assert aug.controller is None                                     # a refused controller attaches nothing
    for kind in ('wgan', 'lsgan'):                                    # the sign of the real scores says nothing there: either order is refused
        a = pg.Augmenter(device='cpu')
        pg.gan_losses(kind, penalty='gp', augment=a)
        with pytest.raises(ValueError):
            pg.AugmentController(a)
        b = pg.Augmenter(device='cpu')
        pg.AugmentController(b)
        with pytest.raises(ValueError):
            pg.gan_losses(kind, penalty='gp', augment=b)
    for kind in ('logistic', 'hinge'):
        a = pg.Augmenter(device='cpu')
        pg.gan_losses(kind, penalty='r1', augment=a)
        c = pg.AugmentController(a)
        assert a.controller is c
        with pytest.raises(ValueError):
            pg.AugmentController(a)                                   # one controller per Augmenter
    with pytest.raises(ValueError):
        pg.gan_losses('logistic', augment='yes')


class _Trainer(object):
    def __init__(self):
        self.cur_nimg, self.stats = 0, {}


def test_controller_rule_on_a_stub_accumulator():
    aug = pg.Augmenter(p=0.5, device='cpu')
    ctl = pg.AugmentController(aug, target=0.6, adjust_kimg=1, interval=4, p_max=0.8)
    assert ctl.trigger_interval == [(4, 'iteration')]
    tr = _Trainer()
    aug.acc[0], aug.acc[1], tr.cur_nimg = 10.0, 20.0, 64               # what was counted before the plugin is registered does not count
    ctl.register(tr)
    assert tr.stats['augment_p']['val'] == 0.5 and np.isnan(tr.stats['augment_rt']['val'])
    for name in ('augment_p', 'augment_rt'):
        assert tr.stats[name]['log_name'] == name and tr.stats[name]['log_epoch_fields'] == ['{val:.4f}']

    def step(d_signs, d_count, d_nimg):
        aug.acc[0] += d_signs
        aug.acc[1] += d_count
        tr.cur_nimg += d_nimg
        ctl.iteration(0)
        return tr.stats['augment_p']['val'], tr.stats['augment_rt']['val']
    up = 0.5 + 64 / (1000.0 * 1.0)
    assert step(16, 16, 64) == (up, 1.0) and aug.p == up                            # r_t = 1 > 0.6: up by images / (1000 adjust_kimg)
    down = up - 100 / (1000.0 * 1.0)
    assert step(-4, 16, 100) == (down, -0.25) and 0.46 < down < 0.47                # r_t < target: down
    assert step(0, 0, 50) == (down, -0.25)                                          # nothing counted: nothing moves ...
    assert step(6, 10, 50) == (down, 0.6)                                           # r_t == target: sign 0 (over the 100 images since the last read that counted)
    assert step(10, 10, 1000) == (0.8, 1.0)                                         # clipped to p_max
    assert step(-10, 10, 5000) == (0.0, -1.0)                                       # ... and to 0
    assert ctl.r_t == -1.0 and aug.read() == (10 + 16 - 4 + 6 + 10 - 10, 20 + 16 + 16 + 10 + 10 + 10)


# ------------------------------------------------------------------------------------------ objectives
def test_gan_losses_with_an_augmenter_never_returns_the_pinned_pair():
    wl = pg.wgan_gp_loss
    aug = pg.Augmenter(device='cpu')
    assert pg.gan_losses('wgan', penalty='gp') == (wl.wgan_gp_D_loss, wl.wgan_gp_G_loss)
    d, g = pg.gan_losses('wgan', penalty='gp', augment=aug)
    assert d is not wl.wgan_gp_D_loss and g is not wl.wgan_gp_G_loss
    assert d.objective is g.objective and d.objective.augment is aug and d.objective.family == 'pinned' and aug.kind == 'wgan'
    assert d.objective[:5] == pg.engine.WGAN_GP[:5]
    d2, _ = pg.gan_losses('wgan', penalty='gp', augment=pg.Augmenter(device='cpu'))
    assert d2.objective != d.objective and hash(d.objective) == hash(tuple(d.objective))      # hashed (and compared) by the Augmenter's identity
    assert len({d.objective, d2.objective, d.objective._replace()}) == 2


def test_objective_without_the_field_is_what_it_was():
    O = pg.engine.Objective
    assert O._fields == ('kind', 'drift', 'penalty', 'weight', 'target', 'family', 'augment')
    assert O('logistic', 0.0, 'r1', 10.0, 1.0) == O('logistic', 0.0, 'r1', 10.0, 1.0, 'pinned', None)
    d, _ = pg.gan_losses('logistic', penalty='r1')
    assert d.objective == O('logistic', 0.0, 'r1', 10.0, 1.0) and d.objective.augment is None       # (what tests/test_gan_losses_host.py builds)
    assert pg.engine.WGAN_GP == O('wgan', 0.001, 'gp', 10.0, 1.0, 'original') and pg.engine.WGAN_GP.augment is None


# ------------------------------------------------------------------------------------------ the step hooks, on the CPU emulation of the kernels
@pytest.fixture()
def emu(monkeypatch):
    for name in ('gan_d_loss', 'gan_g_loss', 'r1_seed'):             # (as in tests/test_gan_losses_host.py)
        monkeypatch.setattr(emu_ops, name, getattr(emu_gan_losses, name), raising=False)
    for modname in ('engine', 'optim'):
        monkeypatch.setattr(importlib.import_module('pggan-pytorch_amd.' + modname), 'ops', emu_ops)
    monkeypatch.setattr(pg.engine, '_check_dev', lambda t, what: t.contiguous())
    # the four augmentation launches as their numpy twins (tensors in, tensors out), beside the emulation of every other kernel
    calls = []

    def apply(x, table, channel_mask=0, out=None):
        calls.append('apply')
        y = torch.from_numpy(A.apply_host(x.numpy(), table.numpy(), channel_mask))
        return y if out is None else out.copy_(y)

    def adjoint(g, table, out=None):
        calls.append('adjoint')
        y = torch.from_numpy(A.adjoint_host(g.numpy(), table.numpy()))
        return y if out is None else out.copy_(y)

    def signs(s, acc):
        calls.append('signs')
        acc[0] += float(torch.sign(s).sum())
        acc[1] += s.numel()
    for name, fn in (('augment_apply', apply), ('augment_adjoint', adjoint), ('score_signs', signs), ('AUGMENT_COLS', 8)):
        monkeypatch.setattr(emu_ops, name, fn, raising=False)
    yield calls


def _nets(name):
    meta, data = load_fixture(name)
    G, D = build_nets(meta)
    load_fixture_params(G, data, 'G')
    load_fixture_params(D, data, 'D')
    c = meta['cfg']
    cfg = ar.oc.NetCfg(c['resolution'], c['num_channels'], fmap_base=c['fmap_base'], fmap_decay=c['fmap_decay'], fmap_max=c['fmap_max'],
                       latent_size=c['latent_size'])
    return G, D, fixture_params(data, 'G'), fixture_params(data, 'D'), cfg


@pytest.mark.parametrize('kind,penalty,name,alpha', [('logistic', 'r1', 'tiny16c1', 1.0), ('hinge', None, 'tiny16c1', 0.5), ('wgan', 'gp', 'tiny32', 1.0)])
def test_steps_on_the_emulation_against_float64_autograd(emu, monkeypatch, kind, penalty, name, alpha):
    """The hooks of engine.d_loss_forward / _d_plain_loss_forward / g_loss_forward / g_loss_backward with injected tables, on the CPU
    emulation: losses and every gradient of D and G against autograd through the oracle's networks with the augmentation inserted
    (bounds of tests/test_engine_host.py).  Without the transpose in the G backward the G gradients miss theirs."""
    from test_engine_host import GRAD_TOL, OUT_TOL
    G, D, gp, dp, cfg = _nets(name)
    depth, n = cfg.max_depth, 3
    G.depth = D.depth = depth
    G.alpha = D.alpha = alpha
    drift = 0.001 if kind == 'wgan' else 0.0
    real, z_d, z_g, mix = synthetic(41, n, cfg.num_channels, cfg.resolution, cfg.latent_size)
    aug = pg.Augmenter(gain=0.3, gain_channels=(0,), device='cpu')
    if kind != 'wgan':
        pg.AugmentController(aug)
    td, tg = ar.step_table(2 * n, cfg.resolution, cfg.resolution, 1), ar.step_table(n, cfg.resolution, cfg.resolution, 2)
    want = ar.d_loss_and_grads(dp, gp, cfg, real, z_d, mix, depth, alpha, kind, drift, penalty, 10.0, td, aug.channel_mask)
    gwant = ar.g_loss_and_grads(gp, dp, cfg, z_g, depth, alpha, kind, tg, aug.channel_mask)
    if kind == 'hinge':
        assert float((1 - want['s_r']).abs().min()) > 1e-3 and float((1 + want['s_f']).abs().min()) > 1e-3
    D_loss, G_loss = pg.gan_losses(kind, penalty=penalty, augment=aug)
    if penalty == 'gp':
        pg.wgan_gp_loss.set_mixing_factors(mix)
    aug.inject(d_table=td, g_table=tg)
    d_cost, d_real, d_fake = D_loss(D, G, real, z_d)
    assert emu == ['apply', 'apply'] + (['signs'] if kind != 'wgan' else []) and aug.draws == {'d': 0, 'g': 0}
    if kind != 'wgan':
        assert aug.read() == (float(torch.sign(want['s_r']).sum()), float(n))
    assert max(rel_err(d_cost, want['d_cost']), rel_err(d_real, want['R']), rel_err(d_fake, want['F'])) < OUT_TOL
    d_cost.backward()
    mine = reference_grads(D)
    assert sorted(mine) == sorted(want['grads'])
    derr = {k: ar.go.grad_err(k, mine[k], r, want['bias_terms']) for k, r in want['grads'].items()}
    assert max(derr.values()) < GRAD_TOL, derr
    del emu[:]
    g_cost = G_loss(G, D, z_g)
    assert rel_err(g_cost, gwant['g_cost']) < OUT_TOL
    g_cost.backward()
    assert emu == ['apply', 'adjoint']
    mine = reference_grads(G)
    assert sorted(mine) == sorted(gwant['grads'])
    gerr = {k: rel_err(mine[k], r) for k, r in gwant['grads'].items()}
    assert max(gerr.values()) < GRAD_TOL, gerr
    # control: the identity in the transpose's place
    monkeypatch.setattr(emu_ops, 'augment_adjoint', lambda g, table, out=None: g)
    aug.inject(g_table=tg)
    G_loss(G, D, z_g).backward()
    mine = reference_grads(G)
    assert max(rel_err(mine[k], r) for k, r in gwant['grads'].items()) > 10 * GRAD_TOL


def test_a_step_needs_its_table_and_an_unaugmented_one_takes_none(emu):
    G, D, _, _, cfg = _nets('tiny16c1')
    G.depth = D.depth = 2
    real, z_d, z_g, mix = synthetic(41, 2, 1, 16, cfg.latent_size)
    aug = pg.Augmenter(device='cpu')
    obj = pg.engine.Objective('logistic', 0.0, 'r1', 10.0, 1.0, augment=aug)
    with pytest.raises(ValueError):
        pg.engine.d_loss_forward(D, G, real, z_d, mix.view(-1), obj)
    with pytest.raises(ValueError):
        pg.engine.g_loss_forward(G, D, z_g, obj, torch.zeros((3, 8), dtype=torch.int32))
    with pytest.raises(ValueError):
        pg.engine.g_loss_forward(G, D, z_g, obj._replace(augment=None), torch.zeros((2, 8), dtype=torch.int32))
    assert emu == []
