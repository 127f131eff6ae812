"""Canonical launch trace of one D step + one G step: what a refactor of the schedules in engine.py must leave byte-identical.

    python tools/launch_trace.py [--emu] [--loss KIND[:PENALTY]] [--out DIR] [--list] [CONFIG ...]

For every named configuration (all of them by default) the networks are built from a fixed seed, ``D_loss(...).backward()`` and
``G_loss(...).backward()`` run eagerly three times, and the third iteration is written to DIR/<mode>_<config>.txt.  The pair is
``wgan_gp_D_loss`` / ``wgan_gp_G_loss`` unless ``--loss`` names another objective: ``pg.gan_losses(KIND, penalty=PENALTY)`` with its
default weights (``--loss hinge``: no penalty; ``--loss logistic:r1``).  Give every ``--loss`` a directory of its own.

  device mode   the iteration runs inside ``plans._Recorder`` on a fresh plan: every C-ABI call by name with all its arguments, every event
                record / wait and the PENDING / BWD_COPIES markers, in issue order.  Scalars are printed verbatim; pointers (the stream
                included) as the ordinal of the first appearance of their value, so the aliasing pattern is kept and the addresses are not
                (the recorder keeps every tensor alive: no address is handed out twice inside a trace).
  --emu         ``engine.ops`` is a proxy around tests/emu_ops.py that logs every call: name, shape and dtype of tensor arguments, scalars
                (arguments bound to the signature, defaults filled in).  Needs no GPU.

``trainer_*`` configurations (device mode, the default pair only) run ``Trainer.train()`` four times with launch plans instead and print ``plans.STATS`` and the
canonical entries of the recorded D and G plans.  Every trace ends with ``dict(engine.FALLBACKS)``.

Comparing two commits: copy this file into a checkout of the other one (it uses only interfaces both have), run both with the same
arguments and ``diff -r`` the two directories."""
import argparse
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import pggan_amd as pg

_lib, engine, plans = pg._lib, pg.engine, pg.plans

WIDE, LAZY, PN = dict(fmap_base=256, fmap_max=64), dict(fmap_base=512, fmap_max=64), dict(fmap_base=128, fmap_max=32)
BYTES8 = dict(SIGN_BYTES_MIN_H=8)


def _configs():
    """name -> (modes, network spec, [(depth, alpha, n, seed)], engine switches)"""
    import json
    out = {}
    for fx in ('tiny32', 'tiny16c1', 'thin1024'):
        with open(os.path.join(ROOT, 'tests', 'golden', fx + '.json')) as f:
            cases = [(c['depth'], c['alpha'], c['n'], c['seed']) for c in json.load(f)['cases']]
        if fx == 'thin1024':
            out[fx] = ('d', fx, [c for c in cases if c[0] >= 7], {})
        else:
            out[fx] = ('ed', fx, cases, {})
    st32 = [(2, 1.0, 2, 302), (3, 0.6, 2, 303)]
    out['wide32'] = ('ed', (32, WIDE, False), st32, {})
    out['wide32_bytes8_wino'] = ('ed', (32, WIDE, False), st32, dict(BYTES8, WINO_MIN_WORKGROUPS=0))
    out['pn32'] = ('ed', (32, PN, True), [(0, 1.0, 4, 300), (1, 0.6, 3, 301), (2, 1.0, 2, 302), (3, 0.3, 2, 303)], {})
    st64 = [(3, 1.0, 3, 303), (4, 0.6, 2, 304), (4, 1.0, 2, 304)]
    out['wide64_bytes8'] = ('d', (64, WIDE, False), st64, BYTES8)
    out['wide64_bytes8_direct'] = ('d', (64, WIDE, False), st64, dict(BYTES8, USE_WINOGRAD=False))
    out['lazy128'] = ('d', (128, LAZY, False), [(5, 1.0, 2, 305), (5, 0.5, 2, 305)], {})
    out['trainer_lazy128'] = ('t', (128, LAZY, False), [(5, 1.0, 2, 305)], {})
    return out


def _nets(spec, dev):
    torch.manual_seed(21)
    if isinstance(spec, str):
        from conftest import load_fixture
        from helpers import build_nets, load_fixture_params
        meta, data = load_fixture(spec)
        G, D = build_nets(meta, dev)
        load_fixture_params(G, data, 'G')
        load_fixture_params(D, data, 'D')
        return G, D
    res, kw, pn = spec
    G = pg.Generator((1, 3, res, res), latent_size=64, **kw)
    D = pg.Discriminator((1, 3, res, res), pixelnorm=True, **kw) if pn else pg.Discriminator((1, 3, res, res), **kw)
    return G.to(dev), D.to(dev)


def _batch(seed, n, C, res, latent, dev):
    rs = np.random.RandomState(seed)
    real = rs.rand(n, C, res, res).astype(np.float32) * 2 - 1
    z_d, z_g = rs.randn(n, latent).astype(np.float32), rs.randn(n, latent).astype(np.float32)
    mix = rs.rand(n, 1).astype(np.float32)
    return tuple(torch.from_numpy(a).to(dev) for a in (real, z_d, z_g, mix))


LOSS = None                    # --loss: (kind, penalty); None: the WGAN-GP pair


def _step(G, D, batch):
    real, z_d, z_g, mix = batch
    D_loss, G_loss = (pg.wgan_gp_D_loss, pg.wgan_gp_G_loss) if LOSS is None else pg.gan_losses(LOSS[0], penalty=LOSS[1])
    if LOSS is None or LOSS[1] == 'gp':                 # ('r1' and no penalty leave an injected draw where it is)
        pg.wgan_gp_loss.set_mixing_factors(mix)
    D_loss(D, G, real, z_d)[0].backward()
    G_loss(G, D, z_g).backward()


class _Ordinals(dict):
    def __call__(self, prefix, v):
        return 'null' if v is None else '%s%d' % (prefix, self.setdefault((prefix, v), len(self)))


def canonical(entries, nets):
    """Text lines of a list of plans._Recorder entries."""
    o = _Ordinals()
    sigs = {}
    for k in sorted(vars(_lib)):                        # the tables of every ABI header (SIGNATURES, GAN_SIGNATURES, ...)
        if k.endswith('SIGNATURES'):
            sigs.update(getattr(_lib, k))
    name_of = dict((id(net), k) for k, net in nets.items())
    lines = []
    for e in entries:
        if e[0] == plans.CALL:
            args = [o('p', a) if t is _lib.P else repr(a) for a, t in zip(e[2], sigs[e[3]])]
            assert len(args) == len(e[2])
            lines.append('%s(%s)' % (e[3], ', '.join(args)))
        elif e[0] in (plans.RECORD, plans.WAIT):
            lines.append('%s %s %s' % ('record' if e[0] == plans.RECORD else 'wait', o('e', id(e[1])), o('p', e[2].cuda_stream)))
        else:
            lines.append('%s %s %s' % ('PENDING' if e[0] == plans.PENDING else 'BWD_COPIES', name_of.get(id(e[1]), '?'), o('p', e[2].cuda_stream)))
    return lines


def _show(v):
    if torch.is_tensor(v):
        return '%s%s' % (str(v.dtype).replace('torch.', ''), list(v.shape))
    if isinstance(v, (list, tuple)):
        return '[%s]' % ', '.join(_show(x) for x in v)
    return repr(v)


class _EmuProxy(object):
    """Stands in for the ``ops`` module: tests/emu_ops.py with every call from the engine logged."""

    def __init__(self, mod, log):
        self._mod, self._log = mod, log

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not inspect.isfunction(fn):
            return fn

        def logged(*a, **k):
            b = inspect.signature(fn).bind(*a, **k)
            b.apply_defaults()
            self._log.append('%s(%s)' % (name, ', '.join('%s=%s' % (p, _show(v)) for p, v in b.arguments.items())))
            return fn(*a, **k)
        return logged


def trace(name, emu):
    modes, spec, stages, switches = _configs()[name]
    dev = 'cpu' if emu else 'cuda'
    saved = dict((k, getattr(engine, k)) for k in switches)
    for k, v in switches.items():
        setattr(engine, k, v)
    engine.FALLBACKS.clear()
    pg.wgan_gp_loss.enable_graphs('auto' if modes == 't' else False)
    lines = []
    try:
        for depth, alpha, n, seed in stages:
            lines.append('== depth %d alpha %r n %d' % (depth, alpha, n))
            if modes == 't':
                import bench
                torch.manual_seed(1337)
                tr = bench.make_trainer(pg, spec[0], depth, alpha, n, 1337, None, fmap_base=spec[1]['fmap_base'])
                plans.clear()
                before = dict(plans.STATS)
                for _ in range(4):
                    tr.train()
                torch.cuda.synchronize()
                lines.append('plans.STATS %r' % dict((k, plans.STATS[k] - before[k]) for k in sorted(before)))
                for key, plan in plans._CACHE.items():
                    lines.append('-- %s plan' % (key[0] if isinstance(key[0], str) else key[0][0]))      # (the step leads the key, or its stage part)
                    lines += canonical(plan.entries or [], dict(D=tr.D, G=tr.G))
                continue
            G, D = _nets(spec, dev)
            G.depth = D.depth = depth
            G.alpha = D.alpha = alpha
            batch = _batch(seed, n, D.num_channels, 4 * 2 ** depth, G.latent_size, dev)
            for _ in range(2):
                _step(G, D, batch)
            if emu:
                real_ops, engine.ops = engine.ops, _EmuProxy(engine.ops, lines)
                try:
                    _step(G, D, batch)
                finally:
                    engine.ops = real_ops
            else:
                with plans._Recorder(plans._Plan()) as rec:
                    _step(G, D, batch)
                torch.cuda.synchronize()
                lines += canonical(rec.entries, dict(D=D, G=G))
    finally:
        for k, v in saved.items():
            setattr(engine, k, v)
    lines.append('FALLBACKS %r' % dict(sorted(engine.FALLBACKS.items())))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--emu', action='store_true', help='host mode: log the calls into tests/emu_ops.py (no GPU)')
    ap.add_argument('--loss', metavar='KIND[:PENALTY]', help="the objective, as pg.gan_losses names it ('hinge', 'logistic:r1'); default: the WGAN-GP pair")
    ap.add_argument('--out', default='launch_trace', help='directory the traces are written to')
    ap.add_argument('--list', action='store_true')
    ap.add_argument('configs', nargs='*')
    a = ap.parse_args()
    if a.loss:
        global LOSS
        LOSS = tuple((a.loss.split(':') + [None])[:2])
    cfgs = _configs()
    mode = 'e' if a.emu else 'd'
    names = a.configs or [k for k, v in cfgs.items() if mode in v[0] or (not a.emu and v[0] == 't' and LOSS is None)]
    if a.list:
        print('\n'.join('%-24s %s' % (k, cfgs[k][0]) for k in names))
        return
    if a.emu:
        import emu_gan_losses
        import emu_ops
        for name in ('gan_d_loss', 'gan_g_loss', 'r1_seed'):        # (as the ``emu`` fixture of tests/test_gan_losses_host.py does)
            setattr(emu_ops, name, getattr(emu_gan_losses, name))
        engine.ops = emu_ops
        engine._check_dev = lambda t, what: t.contiguous()
    os.makedirs(a.out, exist_ok=True)
    for name in names:
        lines = trace(name, a.emu)
        with open(os.path.join(a.out, '%s_%s.txt' % ('emu' if a.emu else 'dev', name)), 'w') as f:
            f.write('\n'.join(lines) + '\n')
        print('%-24s %6d lines' % (name, len(lines)), flush=True)


if __name__ == '__main__':
    main()
