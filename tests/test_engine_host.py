"""Host-side logic of the product (engine schedules, modules, losses, Trainer, DepthManager,
FusedAdam) checked on CPU against the golden fixtures exported from the reference.

The HIP kernels are replaced by ``tests/emu_ops.py`` (a torch-CPU statement of each kernel's
contract, test infrastructure only) through monkeypatching, so what is verified here is everything
ABOVE the C-ABI: the hand-derived gradient-penalty double backward, the batched [real|fake|mixed]
sweep with the minibatch-stddev Hessian-vector injection, active-parameter sets, optimizer and
schedules.  The kernels themselves are verified on the GPU (tests/test_kernels_gpu.py)."""
import importlib
import json

import numpy as np
import pytest
import torch

import emu_ops
from conftest import load_fixture, rel_err
from helpers import (TRACE_MOVEMENT_TOL_HOST, build_flag_nets, build_nets, load_fixture_params, reference_grads, synthetic,
                     trace_movement_errors)

import pggan_amd as pg

OUT_TOL = 2e-4     # G/D outputs and losses: rel. max-norm (north-star bound: 1e-3)
GRAD_TOL = 1e-3    # parameter gradients: rel. max-norm per tensor


@pytest.fixture()
def emu(monkeypatch):
    for modname in ('engine', 'optim'):
        mod = importlib.import_module('pggan-pytorch_amd.' + modname)
        monkeypatch.setattr(mod, 'ops', emu_ops)
    monkeypatch.setattr(pg.engine, '_check_dev', lambda t, what: t.contiguous())
    yield


@pytest.mark.parametrize('name', ['tiny32', 'tiny16c1', 'thin1024'])
def test_schedules_match_reference(emu, name):
    meta, data = load_fixture(name)
    G, D = build_nets(meta)
    load_fixture_params(G, data, 'G')
    load_fixture_params(D, data, 'D')
    cfg = meta['cfg']
    for case in meta['cases']:
        tag, depth, alpha, n = case['tag'], case['depth'], case['alpha'], case['n']
        if name == 'thin1024' and depth > 5:
            continue                                        # CPU time; the GPU suite covers depth 7/8
        real, z_d, z_g, mix = synthetic(case['seed'], n, cfg['num_channels'], 4 * 2 ** depth, cfg['latent_size'])
        G.depth = D.depth = depth
        G.alpha = D.alpha = alpha
        if tag + '/G_out' in data.files:
            assert rel_err(G(z_d), data[tag + '/G_out']) < OUT_TOL
        assert rel_err(D(real), data[tag + '/D_real']) < OUT_TOL
        pg.wgan_gp_loss.set_mixing_factors(mix)
        d_cost, d_real_loss, d_fake_loss = pg.wgan_gp_D_loss(D, G, real, z_d)
        assert rel_err(d_cost, data[tag + '/D_cost']) < OUT_TOL
        assert rel_err(d_real_loss, data[tag + '/D_real_loss']) < OUT_TOL
        assert rel_err(d_fake_loss, data[tag + '/D_fake_loss']) < OUT_TOL
        d_cost.backward()
        mine = reference_grads(D)
        ref = sorted(k[len(tag + '/Dgrad/'):] for k in data.files if k.startswith(tag + '/Dgrad/'))
        assert sorted(mine.keys()) == ref, 'active-parameter set differs'
        for k in ref:
            assert rel_err(mine[k], data['%s/Dgrad/%s' % (tag, k)]) < GRAD_TOL, (tag, k)
        assert all(p.grad is None for p in G.parameters())
        g_cost = pg.wgan_gp_G_loss(G, D, z_g)
        assert rel_err(g_cost, data[tag + '/G_cost']) < OUT_TOL
        g_cost.backward()
        mine = reference_grads(G)
        ref = sorted(k[len(tag + '/Ggrad/'):] for k in data.files if k.startswith(tag + '/Ggrad/'))
        assert sorted(mine.keys()) == ref
        for k in ref:
            assert rel_err(mine[k], data['%s/Ggrad/%s' % (tag, k)]) < GRAD_TOL, (tag, k)


def test_non_default_flags_fixture(emu):
    """ReLU / no wscale / no PixelNorm+latent-normalisation variants against the reference's own run."""
    meta, data = load_fixture('flags16')
    for case in meta['cases']:
        tag = case['tag']
        G, D = build_flag_nets(meta, case)
        load_fixture_params(G, data, tag + '/G')
        load_fixture_params(D, data, tag + '/D')
        G.depth = D.depth = case['depth']
        G.alpha = D.alpha = case['alpha']
        real, z_d, z_g, mix = synthetic(case['seed'], case['n'], 3, 16, 32)
        assert rel_err(G(z_d), data[tag + '/G_out']) < OUT_TOL
        assert rel_err(D(real), data[tag + '/D_real']) < OUT_TOL
        pg.wgan_gp_loss.set_mixing_factors(mix)
        d_cost, _, _ = pg.wgan_gp_D_loss(D, G, real, z_d)
        assert rel_err(d_cost, data[tag + '/D_cost']) < OUT_TOL
        d_cost.backward()
        mine = reference_grads(D)
        for k in data.files:
            if k.startswith(tag + '/Dgrad/'):
                assert rel_err(mine[k.split('/', 2)[2]], data[k]) < GRAD_TOL, k
        g_cost = pg.wgan_gp_G_loss(G, D, z_g)
        assert rel_err(g_cost, data[tag + '/G_cost']) < OUT_TOL
        g_cost.backward()
        mine = reference_grads(G)
        for k in data.files:
            if k.startswith(tag + '/Ggrad/'):
                assert rel_err(mine[k.split('/', 2)[2]], data[k]) < GRAD_TOL, k
    # wscale=False construction keeps equalized lr on the to/fromRGB layers, like the reference
    torch.manual_seed(41)
    G, D = build_flag_nets(meta, meta['cases'][1])
    for pre, net in (('nowscale/G', G), ('nowscale/D', D)):
        for k, v in net.reference_state_dict().items():
            ref = data['%s/%s' % (pre, k)]
            if torch.is_tensor(v):
                assert torch.equal(v, torch.from_numpy(ref)), k
            else:
                assert np.float32(v) == np.float32(ref), k


def test_init_matches_reference_bit_exact():
    """Same seed, same construction order => same weights as the reference (network.py:8-30)."""
    for name in ('tiny32', 'tiny16c1'):
        meta, data = load_fixture(name)
        torch.manual_seed(meta['init_seed'])
        G, D = build_nets(meta)
        for pre, net in (('G', G), ('D', D)):
            sd = net.reference_state_dict()
            for k, v in sd.items():
                ref = data['%s/%s' % (pre, k)]
                if torch.is_tensor(v):
                    assert torch.equal(v, torch.from_numpy(ref)), k
                else:
                    assert np.float32(v) == np.float32(ref), k


def run_trainer_trace(check_losses=True, losses_out=None):
    """Trainer + DepthManager + LRScheduler + FusedAdam over the 14 iterations of tests/golden/trace16.* on the emulated ops (the ``emu``
    fixture must be active): (meta, data, G, D) after the last iteration.  ``check_losses=False`` leaves the per-iteration loss
    assertions out (tests/test_optimizer_host.py runs the trace with a deliberately mis-scaled step); ``losses_out`` receives the recorded
    losses, {'G': [...], 'D': [...]}."""
    meta, data = load_fixture('trace16')
    G, D = build_nets(meta)
    load_fixture_params(G, data, 'G0')
    load_fixture_params(D, data, 'D0')
    opt_g = pg.FusedAdam(G.parameters(), 0.001, betas=(0.0, 0.99))
    opt_d = pg.FusedAdam(D.parameters(), 0.001, betas=(0.0, 0.99))
    rk = meta['lr_rampup_kimg']
    ramp = lambda nimg: pg.utils.rampup(nimg, rk)
    lrs_d, lrs_g = pg.RampupLR(opt_d, ramp), pg.RampupLR(opt_g, ramp)
    cnt = dict(real=0, z=0, mix=0)

    class Data(object):
        model_depth = 0
        alpha = 1.0
    dataset = Data()

    def make_loader(mb):
        def gen():
            while True:
                x = torch.from_numpy(data['real/%d' % cnt['real']])
                cnt['real'] += 1
                assert x.shape[0] == mb and x.shape[-1] == 4 * 2 ** dataset.model_depth
                yield x
        return gen()

    def make_rlg(mb):
        def f():
            z = torch.from_numpy(data['z/%d' % cnt['z']])
            cnt['z'] += 1
            assert z.shape[0] == mb
            return z
        return f

    def d_loss(Dm, Gm, real, z):
        pg.wgan_gp_loss.set_mixing_factors(torch.from_numpy(data['mix/%d' % cnt['mix']]))
        cnt['mix'] += 1
        return pg.wgan_gp_D_loss(Dm, Gm, real, z)

    tr = pg.Trainer(D, G, d_loss, pg.wgan_gp_G_loss, opt_d, opt_g, dataset, make_loader(4), make_rlg(4))
    pg.trainer._to_device = lambda t: t
    dm_kw = {k: ({int(a): b for a, b in v.items()} if isinstance(v, dict) else v) for k, v in meta['dm_kw'].items()}
    tr.register_plugin(pg.DepthManager(make_loader, make_rlg, 2, **dm_kw))
    tr.register_plugin(pg.LRScheduler(lrs_d, lrs_g))
    losses = dict(G=[], D=[])

    class Rec(pg.Plugin):
        def __init__(self):
            super(Rec, self).__init__([(1, 'iteration')])

        def register(self, trainer):
            pass

        def iteration(self, i, g_cost, d_cost, d_real, d_fake):
            losses['G'].append(float(g_cost))
            losses['D'].append(float(d_cost))
    tr.register_plugin(Rec())
    import heapq
    for q in tr.plugin_queues.values():
        heapq.heapify(q)
    for it in range(meta['n_iter']):
        assert (tr.cur_nimg, G.depth, repr(float(G.alpha))) == (meta['nimg'][it], meta['depth'][it], meta['alpha'][it])
        assert repr(float(opt_d.param_groups[0]['lr'])) == meta['lr'][it]
        tr.train()
        if check_losses:
            assert abs(losses['D'][it] - meta['D_cost'][it]) < 2e-4 * max(1.0, abs(meta['D_cost'][it])), it
            assert abs(losses['G'][it] - meta['G_cost'][it]) < 2e-4 * max(1.0, abs(meta['G_cost'][it])), it
    assert tr.cur_nimg == meta['final_nimg']
    if losses_out is not None:
        losses_out.update(losses)
    return meta, data, G, D


def test_trainer_trace(emu):
    """Trainer + DepthManager + LRScheduler + FusedAdam over 14 iterations (depth 0->2 with fades and a
    minibatch change) against the reference's own run (tests/golden/trace16.*)."""
    meta, data, G, D = run_trainer_trace()
    for pre, net in (('G1', G), ('D1', D)):
        sd = net.reference_state_dict()
        for k, v in sd.items():
            if torch.is_tensor(v):
                assert rel_err(v, data['%s/%s' % (pre, k)]) < 2e-3, k
    # the weights above move by 5e-4 at most on tensors of size 2 .. 4: only the movement itself shows whether the step is right
    moved = trace_movement_errors(data, G=G, D=D)
    print('movement rel-L2 per tensor: max %.2e (%s)' % max((v, k) for k, v in moved.items()))
    assert len(moved) >= 20 and max(moved.values()) < TRACE_MOVEMENT_TOL_HOST, moved


def test_depth_manager_bit_exact():
    with open(__import__('os').path.join(__import__('conftest').GOLDEN, 'schedule.json')) as f:
        sched = json.load(f)

    class Net(object):
        depth, alpha = 0, 1.0

    class Tr(object):
        def __init__(self):
            self.cur_nimg = 0
            self.D, self.G, self.dataset = Net(), Net(), Net()
            self.dataset.model_depth = 0
            self.stats = {}
            self.tick_duration_nimg = 0
    for sw in sched['sweeps']:
        kw = {k: ({int(a): b for a, b in v.items()} if isinstance(v, dict) else v) for k, v in sw['kw'].items()}
        dm = pg.DepthManager(lambda mb: [mb], lambda mb: (lambda: mb), sw['max_depth'], **kw)
        tr = Tr()
        dm.register(tr)
        for nimg, depth, alpha_repr, mb, tick in sw['table']:
            tr.cur_nimg = nimg
            dm.iteration()
            assert (tr.G.depth, repr(float(tr.G.alpha)), tr.stats['minibatch_size'], tr.tick_duration_nimg) == \
                   (depth, alpha_repr, mb, tick), nimg
    for nimg, lr_repr in sched['lr']:
        assert repr(float(0.001 * pg.utils.rampup(nimg))) == lr_repr


def test_library_exports_every_declared_symbol():
    """The C-ABI library loads and exports every symbol include/*.h declares (no compute): the product boundary
    (pggan_hip.h) and the thread-local diagnostic exports (pggan_hip_debug.h)."""
    import ctypes
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'pggan_hip.h')).read()
    declared = set(re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', hdr))
    assert declared == set(pg._lib.SIGNATURES), declared ^ set(pg._lib.SIGNATURES)
    assert not any(n.startswith('pg_debug') for n in declared)          # the product header carries no debug state
    dbg = open(os.path.join(root, 'include', 'pggan_hip_debug.h')).read()
    declared_dbg = set(re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', dbg))
    assert declared_dbg == set(pg._lib.DEBUG_SIGNATURES), declared_dbg ^ set(pg._lib.DEBUG_SIGNATURES)
    declared |= declared_dbg
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pg_abi_version() == pg._lib.ABI_VERSION


def _library_sources():
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = glob.glob(os.path.join(root, 'pggan-pytorch_amd', 'csrc', '*')) + glob.glob(os.path.join(root, 'include', '*'))
    assert len(paths) > 10
    return root, {p: open(p).read() for p in paths}


def test_library_reads_no_environment_variable():
    """pggan_hip.h lists the library's process-wide state "all of it": no source or header may call getenv."""
    _, srcs = _library_sources()
    assert [p for p, text in srcs.items() if 'getenv' in text] == []


def test_tuning_values_are_named():
    """Every PG_TUNE_* key / PG_PATH_* value that pggan_hip_debug.h declares is interpreted somewhere in csrc/, and csrc/ compares
    g_tune[...] against those names: no bare integer other than 0 and -1 (the "built-in choice" tests)."""
    import os
    import re
    root, srcs = _library_sources()
    dbg = srcs[os.path.join(root, 'include', 'pggan_hip_debug.h')]
    names = re.findall(r'\b(PG_(?:TUNE|PATH)_\w+)\s*=\s*\d+', dbg)
    assert len(names) >= 4 + 7, names
    csrc = '\n'.join(text for p, text in srcs.items() if os.sep + 'csrc' + os.sep in p)
    for name in names:
        assert re.search(r'\b%s\b' % name, csrc), name
    cmp_ops = r'(?:==|!=|<=|>=|<|>)'
    bare = re.findall(r'g_tune\[[^\]]*\]\s*%s\s*(-?\d+)\b' % cmp_ops, csrc) + \
        re.findall(r'(-?\b\d+)\s*%s\s*g_tune\[' % cmp_ops, csrc)
    assert len(bare) >= 3                                    # (the pattern still finds the comparisons)
    assert [v for v in bare if v not in ('0', '-1')] == []
    assert not re.search(r'switch\s*\(g_tune\[[^)]*\)\s*\{[^}]*\bcase\s+-?\d', csrc)


def test_debug_set_wino_accepts_only_existing_variants():
    """pg_debug_set_wino (host-only, thread-local): the first-generation kernel's values 2 and 4 are argument errors."""
    import ctypes
    import os
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(pg.LIB_PATH)
    PG_E_ARG = -1
    try:
        assert lib.pg_debug_set_wino(4) == PG_E_ARG and lib.pg_debug_set_wino(2) == PG_E_ARG
        for v in (0, 11, 12, 20, 21):
            assert lib.pg_debug_set_wino(v) == 0, v
    finally:
        lib.pg_debug_set_wino(0)


def test_no_cpu_fallback():
    meta, data = load_fixture('tiny32')
    G, D = build_nets(meta)
    with pytest.raises(RuntimeError):
        G(torch.zeros(2, 16))
    with pytest.raises(RuntimeError):
        pg.wgan_gp_D_loss(D, G, torch.zeros(2, 3, 4, 4), torch.zeros(2, 16))


def test_bench_refuses_more_gpus_than_visible():
    """``python bench.py --gpus N`` launches the N ranks itself and must not silently measure fewer devices."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    want = torch.cuda.device_count() + 1 if torch.cuda.is_available() else 2
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(max(2, want))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'GPU(s) are visible' in r.stderr, (r.returncode, r.stderr[-300:])
    env['WORLD_SIZE'] = '4'
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'WORLD_SIZE' in r.stderr


def test_time_monitor_stat_names():
    """plugins.TimeMonitor fills the reference's per-tick timing stats (plugins.py:114-139: 'time', 'sec.tick', 'sec.kimg') and this
    project's 'img/s' / 'd_gp_ms'; no device is needed for the host-clock half."""
    from datetime import timedelta

    class T(object):
        cur_nimg = 100
        stats = {}
        d_step_probe = None
    tr = T()
    mon = pg.TimeMonitor(base_time=5, sample_every=4)
    assert mon.trigger_interval == [(1, 'epoch')]
    mon.register(tr)
    assert tr.stats['sec'] == {'log_format': ':.1f'} and tr.d_step_probe == {'every': 4, 'pairs': []}
    tr.cur_nimg = 1100
    mon.epoch(1)
    assert isinstance(tr.stats['time'], timedelta) and tr.stats['time'].total_seconds() >= 5
    assert tr.stats['sec']['tick'] > 0 and abs(tr.stats['sec']['kimg'] - tr.stats['sec']['tick']) < 1e-9       # 1000 images in the tick
    assert abs(tr.stats['img/s']['val'] * tr.stats['sec']['tick'] - 1000) < 1e-6
    assert tr.stats['d_gp_ms']['val'] == 0.0                 # (no sampled iteration: the probe needs device events)


def test_process_group_handle_is_not_pickled():
    """SaverPlugin pickles whole modules (plugins.py:155-166).  In the exact-global stddev mode the Discriminator holds the data-parallel
    group (communicator handle, streams): it must stay out of the pickle, and a reloaded network starts in the local-shard mode."""
    import io

    class Handle(object):
        def __reduce__(self):
            raise RuntimeError('the process-group handle must not be pickled')
    D = pg.Discriminator((1, 3, 16, 16), fmap_base=64, fmap_max=16)
    D._rt.global_stddev = Handle()
    buf = io.BytesIO()
    torch.save(D, buf)
    buf.seek(0)
    D2 = torch.load(buf, weights_only=False)
    assert D2._rt.global_stddev is None and '_global_stddev' not in vars(D2) and isinstance(D._rt.global_stddev, Handle)


SCHEDULE_KEYS = ('_derived_ver', '_derived_live', '_derived_ev', '_derived_waited', '_derived_bwd_ev', '_derived_bwd_waited', '_bwd_wanted',
                 '_defer_active', '_pending_ev', '_pending', '_skip_join', '_plan_unjoined', '_grad_hook', '_grad_exchange',
                 '_global_stddev', '_gs_checked', '_early_g_request', '_early_fwd', '_d_fwd_buffers')       # where the schedule state lived before runtime.NetRuntime
HOST_CACHES = {'_plist', '_layer_list', '_torch_versions_seen'}      # the only attributes a network may gain while it runs


def _tiny32_after_steps():
    meta, data = load_fixture('tiny32')
    G, D = build_nets(meta)
    cfg = meta['cfg']
    for net in (G, D):
        net._ensure_buffers()
    keys = {id(m): set(vars(m)) for net in (G, D) for m in [net] + net._layers()}
    for alpha in (1.0, 0.5):
        G.depth = D.depth = 2
        G.alpha = D.alpha = alpha
        real, z_d, z_g, mix = synthetic(3, 4, cfg['num_channels'], 16, cfg['latent_size'])
        pg.wgan_gp_loss.set_mixing_factors(mix)
        pg.wgan_gp_D_loss(D, G, real, z_d)[0].backward()
        pg.wgan_gp_G_loss(G, D, z_g).backward()
    return G, D, keys


def test_no_attribute_is_stuck_onto_a_module_at_run_time(emu):
    """The step schedules keep their state in ``net._rt`` (runtime.NetRuntime) and in three attributes every PGConv2d is built with: a D
    step and a G step (fully grown and fading in) leave no new attribute on a layer, and none but the host caches on a network."""
    G, D, keys = _tiny32_after_steps()
    for net in (G, D):
        assert set(vars(net)) - keys[id(net)] <= HOST_CACHES, sorted(set(vars(net)) - keys[id(net)])
        for m in net._layers():
            assert set(vars(m)) == keys[id(m)], sorted(set(vars(m)) - keys[id(m)])


def test_runtime_object_is_closed_and_not_pickled(emu):
    import io
    G, D, _ = _tiny32_after_steps()
    fresh = pg.runtime.NetRuntime()
    for net in (G, D):
        with pytest.raises(AttributeError):
            net._rt.derived_version = None                 # (an undeclared field)
        assert net._rt.derived_ver is not None and net._rt.bwd_wanted          # the steps did leave state behind
        buf = io.BytesIO()
        torch.save(net, buf)
        buf.seek(0)
        net2 = torch.load(buf, weights_only=False)
        for f in fresh.__slots__:
            assert getattr(net2._rt, f) == getattr(fresh, f), f
        assert net._rt.derived_ver is not None             # (the original keeps its own)
        for m in net2._layers():
            assert m._wt_wanted is False and m._wino_wanted is False and m._pending_wgrad is None
    assert any(m._wt_wanted for m in D._layers())


def test_snapshot_with_loose_schedule_attributes_loads():
    """A whole-module snapshot of an earlier version carries the schedule state as loose attributes (reset to None / False / empty when it
    was written): they are dropped on load."""
    D = pg.Discriminator((1, 3, 16, 16), fmap_base=64, fmap_max=16)
    state = D.__getstate__()
    assert '_rt' not in state and not set(SCHEDULE_KEYS) & set(state)
    for k in SCHEDULE_KEYS:
        state[k] = set() if k.endswith('_waited') else False if k in ('_skip_join', '_plan_unjoined', '_defer_active', '_bwd_wanted') else None
    D2 = pg.Discriminator.__new__(pg.Discriminator)
    D2.__setstate__(state)
    assert not set(SCHEDULE_KEYS) & set(vars(D2)) and isinstance(D2._rt, pg.runtime.NetRuntime)
    lay = D.blocks[0].c1
    lstate = dict(lay.__getstate__(), _wt_ver=None)
    del lstate['_wt_wanted']                               # (set on the first request only; '_wt_ver' was written and never read)
    lay2 = type(lay).__new__(type(lay))
    lay2.__setstate__(lstate)
    assert '_wt_ver' not in vars(lay2) and lay2._wt_wanted is False and lay2._wino_wanted is False and lay2._pending_wgrad is None


# ---- saved-activation records (saved.py) ----------------------------------------------------------------------------------------------
def _record_classes():
    S = pg.saved
    return [c for c in vars(S).values() if isinstance(c, type) and issubclass(c, S._Record) and c is not S._Record]


def _walk(rec):
    """``rec`` and every record it holds (directly or in a list)."""
    yield rec
    for f in rec.__slots__:
        v = getattr(rec, f)
        for r in (v if isinstance(v, list) else [v]):
            if isinstance(r, pg.saved._Record):
                for q in _walk(r):
                    yield q


def _pn_fade_in_nets():
    """The flags16 configuration with a PixelNorm discriminator (the fixture itself holds no such case: no reference values are needed
    here), at the fixture's fade-in stage."""
    meta, _ = load_fixture('flags16')
    torch.manual_seed(5)
    G, D = build_flag_nets(meta, dict(g={}, d={'pixelnorm': True}))
    G.depth = D.depth = 2
    G.alpha = D.alpha = 0.45
    return G, D


def test_saved_records_are_closed_and_every_tensor_slot_has_a_layout(emu, monkeypatch):
    S = pg.saved
    classes = _record_classes()
    assert len(classes) == 9
    for cls in classes:
        assert set(cls.LAYOUT) == set(cls.__slots__) and len(cls.__slots__) == len(cls.LAYOUT), cls      # one table, every field in it
        assert set(cls.LAYOUT.values()) <= {S.IMG, S.PIX, S.GRP, S.EACH, None}, cls
        rec = cls()
        assert not hasattr(rec, '__dict__') and all(getattr(rec, f) is None for f in cls.__slots__)
        with pytest.raises(AttributeError):
            rec.undeclared = 1
        with pytest.raises(AttributeError):
            cls(undeclared=1)
    # what a D step and a G step really store: PixelNorm discriminator while fading in (adjoints, injections, pf, r1 / r2) and the default
    # network with sign bytes (inpb, a1b, byte a2)
    hvps = []
    tangent = pg.engine.d_tangent_wgrad
    monkeypatch.setattr(pg.engine, 'd_tangent_wgrad', lambda *a: hvps.append(tangent(*a)) or hvps[-1])
    monkeypatch.setattr(pg.engine, 'SIGN_BYTES_MIN_H', 8)
    meta, _ = load_fixture('tiny32')
    G2, D2 = build_nets(meta)
    G2.depth = D2.depth = 3
    states = []
    for (G, D), res, latent in ((_pn_fade_in_nets(), 16, 32), ((G2, D2), 32, meta['cfg']['latent_size'])):
        real, z_d, z_g, mix = synthetic(7, 2, 3, res, latent)
        _, _, _, st = pg.engine.d_loss_forward(D, G, real, z_d, mix.view(-1), pg.engine.WGAN_GP)
        pg.engine.d_loss_backward(st)
        _, gst = pg.engine.g_loss_forward(G, D, z_g, pg.engine.WGAN_GP)
        pg.engine.g_loss_backward(gst)
        states += [st, gst]
    assert len(hvps) == 2 and hvps[0].injs is not None and hvps[0].n_head == 4
    seen, tensor_fields = set(), set()
    for top in states + hvps:
        for rec in _walk(top):
            seen.add(type(rec))
            for f in rec.__slots__:                       # the SLOTS, not the table: a tensor in an undeclared-layout slot fails
                if torch.is_tensor(getattr(rec, f)):
                    assert type(rec).LAYOUT[f] in (S.IMG, S.PIX, S.GRP), (type(rec).__name__, f)
                    tensor_fields.add((type(rec).__name__, f))
    assert seen == set(classes)
    for f in ('inpb', 'a1b', 'pf', 'r1', 'r2', 'mb', 'stats'):
        assert ('DBlock', f) in tensor_fields, f
    for f in S.DAdjoint.__slots__ + S.PNInjection.__slots__ + ('tx', 'tstats', 'gy_first'):
        assert any(name == f for _, name in tensor_fields), f


def _assert_row_range(full, sub, n, a, b, g0, g1):
    """Every declared tensor of ``sub`` (and of its block records) is exactly rows [a, b) / groups [g0, g1) of the one in ``full``."""
    S = pg.saved
    checked = set()
    for rf, rs in zip(_walk(full), _walk(sub)):
        assert type(rf) is type(rs)
        for f in rs.__slots__:
            o, s = getattr(rf, f), getattr(rs, f)
            layout = type(rs).LAYOUT[f]
            if not torch.is_tensor(o):
                assert not torch.is_tensor(s) and (layout in (None, S.EACH) or (o is None and s is None)), f
                continue
            if layout == S.GRP:
                lo, hi = g0, g1
                assert o.shape[0] == full.groups
            else:
                assert layout in (S.IMG, S.PIX) and o.shape[0] % n == 0 and (layout == S.PIX or o.shape[0] == n), (f, tuple(o.shape))
                per = o.shape[0] // n
                lo, hi = a * per, b * per
            want = o[lo:hi]
            assert s.shape == want.shape and s.shape[0] == hi - lo < o.shape[0], (f, tuple(s.shape))     # nothing left at full extent
            assert s.untyped_storage().data_ptr() == o.untyped_storage().data_ptr(), f
            assert s.data_ptr() == want.data_ptr() and s.stride() == want.stride() and s.dtype == o.dtype, f
            checked.add(f)
    return checked


def _d_context(config, monkeypatch, n=2):
    if config == 'pixelnorm-fade-in':
        _, D = _pn_fade_in_nets()
        res, covers = 16, {'r1', 'r2', 'pf'}
    else:
        meta, _ = load_fixture('tiny32')
        _, D = build_nets(meta)
        if config == 'sign-bytes':
            monkeypatch.setattr(pg.engine, 'SIGN_BYTES_MIN_H', 8)          # (as tests/test_winograd.py::test_engine_with_sign_bytes_host)
            monkeypatch.setattr(pg.engine, 'USE_SIGN_BYTES', True)
            D.depth, res, covers = 3, 32, {'inpb', 'a1b', 'a2'}
        else:
            D.depth, res, covers = 0, 4, {'mb', 'stats'}
    torch.manual_seed(3)
    x = torch.rand(3 * n, 3, res, res) * 2 - 1
    _, ctx = pg.engine.d_forward(D, x, groups=3)
    if config == 'sign-bytes':
        assert ctx.recs[0].a2.dtype == torch.uint8 and ctx.recs[0].inpb.dtype == torch.uint8 and ctx.recs[0].a1b.dtype == torch.uint8
    if config == 'last-block':
        assert len(ctx.recs) == 1 and ctx.recs[0].last
    return D, x, ctx, covers


D_SLICE_CONFIGS = ['pixelnorm-fade-in', 'sign-bytes', 'last-block']


@pytest.mark.parametrize('config', D_SLICE_CONFIGS)
def test_d_context_slice_is_the_row_range_of_every_declared_tensor(emu, monkeypatch, config):
    n = 2
    _, _, ctx, covers = _d_context(config, monkeypatch, n)
    sub = ctx.slice(2 * n, 3 * n, 2, 3)
    assert (sub.NB, sub.groups, sub.depth, sub.alpha) == (n, 1, ctx.depth, ctx.alpha) and (ctx.NB, ctx.groups) == (3 * n, 3)
    checked = _assert_row_range(ctx, sub, 3 * n, 2 * n, 3 * n, 2, 3)
    assert covers | {'x', 'inp', 'a1', 'a2'} <= checked, checked
    for rf, rs in zip(ctx.recs, sub.recs):
        assert (rs.blk, rs.H, rs.first, rs.last) == (rf.blk, rf.H, rf.first, rf.last)


@pytest.mark.parametrize('config', D_SLICE_CONFIGS)
def test_d_context_merge_round_trip(emu, monkeypatch, config):
    n = 2
    D, x, ctx, _ = _d_context(config, monkeypatch, n)
    for rec in _walk(ctx):                                   # an emulated op may hand out a view of a temporary (PixelNorm's scales); the
        for f in rec.__slots__:                              # device ops and the arena hand out tensors that own their rows
            if torch.is_tensor(getattr(rec, f)) and getattr(rec, f)._base is not None:
                setattr(rec, f, getattr(rec, f).clone())
    parts = [ctx.slice(g * n, (g + 1) * n, g, g + 1) for g in range(3)]
    whole = pg.saved.DContext.merge(parts)
    assert (whole.NB, whole.groups, whole.depth, whole.alpha) == (ctx.NB, ctx.groups, ctx.depth, ctx.alpha)
    count = 0
    for rf, rw in zip(_walk(ctx), _walk(whole)):
        for f in rf.__slots__:
            o, w = getattr(rf, f), getattr(rw, f)
            if torch.is_tensor(o):
                assert w is o, f                              # the original tensors themselves
                count += 1
            elif not isinstance(o, list):
                assert w is o or w == o, f
    assert count >= 4
    # slices of DIFFERENT base tensors (a second pass over the same images) are not one batch
    _, other = pg.engine.d_forward(D, x, groups=3)
    with pytest.raises(RuntimeError, match='did not write into one tensor'):
        pg.saved.DContext.merge([parts[0], other.slice(n, 2 * n, 1, 2), parts[2]])
    with pytest.raises(RuntimeError, match='did not write into one tensor'):
        pg.saved.DContext.merge(parts[:2])                   # (two thirds do not cover the base tensors)


def test_g_context_slice_is_the_row_range_of_every_declared_tensor(emu):
    """The batched early generator pass: one pass over [z | z'], the second half is left for the G step."""
    meta, _ = load_fixture('tiny32')
    G, _ = build_nets(meta)
    G.depth, n = 2, 3
    torch.manual_seed(4)
    z2 = torch.randn(2 * n, meta['cfg']['latent_size'])
    _, ctx = pg.engine.generator_forward(G, z2, save=True)
    sub = ctx.slice(n, 2 * n)
    assert (sub.N, sub.depth, sub.alpha, len(sub.recs)) == (n, 2, ctx.alpha, 2) and ctx.N == 2 * n
    checked = _assert_row_range(ctx, sub, 2 * n, n, 2 * n, None, None)
    assert checked == {'zn', 'y1', 'r1', 'y2', 'r2', 'inp', 'a1', 'a2'}
    assert sub.recs[0].blk is ctx.recs[0].blk and sub.recs[1].H == ctx.recs[1].H == 16
    # enumeration for the cross-stream hand-over: each distinct tensor object once (a block's inp IS the coarser output)
    ts = list(pg.saved.tensors(ctx))
    assert len(ts) == len(set(id(t) for t in ts)) == 5 + 4 * 2 and ctx.recs[0].inp is ctx.y2 and ctx.recs[1].inp is ctx.recs[0].a2


# ---- the sign-byte fallback rule (engine._bytes_first) and the hand-over between D's blocks (saved.PoolAdjoint) --------------------------
def test_bytes_first_rule(emu, monkeypatch):
    eng, S = pg.engine, pg.saved
    monkeypatch.setattr(eng, 'FALLBACKS', type(eng.FALLBACKS)())
    y = torch.tensor([[1.0, -2.0, 3.0, -4.0]])
    f32, by = y.clone(), emu_ops.signbytes_of(y)
    calls = []

    def refusing(mask, bytes_out):                                           # a launch without a byte-aware kernel
        calls.append((mask, bytes_out))
        if bytes_out or (torch.is_tensor(mask) and mask.dtype == torch.uint8):
            raise emu_ops.Unsupported('bytes')
        return 'redone'

    def taking(mask, bytes_out):
        calls.append((mask, bytes_out))
        return 'bytes'

    # refused bytes: counted once under the tag, redone with the fp32 copy AS GIVEN
    assert eng._bytes_first(refusing, S.Sign(f32, by, 0.2), 'tag A') == 'redone'
    assert dict(eng.FALLBACKS) == {'tag A': 1}
    assert [c[0] is m for c, m in zip(calls, (by, f32))] == [True, True] and [c[1] for c in calls] == [False, False]
    # ... bytes only: expanded for the second attempt, and only then
    del calls[:]
    expanded = []
    monkeypatch.setattr(emu_ops, 'signbytes_to_mask', lambda b, _orig=emu_ops.signbytes_to_mask: expanded.append(b) or _orig(b))
    assert eng._bytes_first(refusing, S.Sign(bytes=by), 'tag B') == 'redone'
    assert eng.FALLBACKS['tag B'] == 1 and len(expanded) == 1 and expanded[0] is by
    assert calls[1][0].dtype == torch.float32 and torch.equal(torch.sign(calls[1][0]), torch.sign(y))
    # ... a byte OUTPUT (signs_out / y_bytes) is a request of the same kind: redone without it, the mask unchanged
    del calls[:]
    assert eng._bytes_first(refusing, S.Sign(f32), 'tag C', bytes_out=True) == 'redone'
    assert eng._bytes_first(refusing, None, 'tag C', bytes_out=True) == 'redone'
    assert eng.FALLBACKS['tag C'] == 2 and [(c[0] is f32, c[1]) for c in calls[:2]] == [(True, True), (True, False)]
    assert [c for c in calls[2:]] == [(None, True), (None, False)]
    assert len(expanded) == 1
    # "do not count" (the tangent pass's fromRGB retry)
    n = sum(eng.FALLBACKS.values())
    assert eng._bytes_first(refusing, S.Sign(f32, by), 'tag D', count=False) == 'redone'
    assert sum(eng.FALLBACKS.values()) == n and 'tag D' not in eng.FALLBACKS
    # "redo": called in place of the second attempt (the launch expands the bytes itself), counted all the same; nothing is expanded for it
    del calls[:]
    assert eng._bytes_first(refusing, S.Sign(bytes=by), 'tag D2', redo=lambda: 'own redo') == 'own redo'
    assert len(calls) == 1 and calls[0][0] is by and len(expanded) == 1 and eng.FALLBACKS['tag D2'] == 1
    assert eng._bytes_first(taking, S.Sign(bytes=by), 'tag D2', redo=lambda: 'own redo') == 'bytes' and eng.FALLBACKS['tag D2'] == 1
    # no byte in play: nothing to redo, Unsupported is the caller's -- and nothing is counted
    def unsupported(mask, bytes_out):
        calls.append((mask, bytes_out))
        raise emu_ops.Unsupported('shape')
    for sign in (S.Sign(f32), None):
        del calls[:]
        with pytest.raises(emu_ops.Unsupported):
            eng._bytes_first(unsupported, sign, 'tag E')
        assert len(calls) == 1
    # ... nor when the second attempt is refused as well
    with pytest.raises(emu_ops.Unsupported):
        eng._bytes_first(unsupported, S.Sign(f32, by), 'tag F')
    assert 'tag E' not in eng.FALLBACKS and eng.FALLBACKS['tag F'] == 1
    # the byte call succeeds: one call, nothing counted, nothing expanded
    del calls[:]
    n = sum(eng.FALLBACKS.values())
    assert eng._bytes_first(taking, S.Sign(f32, by), 'tag G') == 'bytes'
    assert len(calls) == 1 and calls[0][0] is by and sum(eng.FALLBACKS.values()) == n and len(expanded) == 1


def test_pool_adjoint_is_evaluated_or_lazy():
    S = pg.saved
    g, by = torch.zeros(1, 2, 2, 4), torch.zeros(1, 4, 4, 1, dtype=torch.uint8)
    assert S.PoolAdjoint(g=g).coarse is None
    lazy = S.PoolAdjoint(coarse=g, up=S.Sign(bytes=by, slope=0.2), mul=0.25)
    assert lazy.g is None and lazy.up.bytes is by
    for bad in (dict(), dict(g=g, coarse=g, up=S.Sign(bytes=by), mul=0.25), dict(g=g, mul=0.25), dict(coarse=g, mul=0.25),
                dict(coarse=g, up=S.Sign(f32=g), mul=0.25), dict(coarse=g, up=S.Sign(bytes=by))):
        with pytest.raises(ValueError):
            S.PoolAdjoint(**bad)
    for rec in (lazy, S.Sign()):
        assert not hasattr(rec, '__dict__')
        with pytest.raises(AttributeError):
            rec.undeclared = 1
