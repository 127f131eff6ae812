"""GPU tier of the latent projection (pggan-pytorch_amd/projection.py, include/pggan_hip_projection.h).

The loss kernel is held to the float64 twin (tests/projection_ref.py) with DERIVED bounds: its sums are fp64, so an output differs from
the twin's by one fp32 rounding (2^-24 relative to the sum of the magnitudes of its terms) plus the fp64 reordering; 2^-23 covers both.
dz is judged on the linear piece the device pass itself selected, as tests/test_fp64_adjudicator.py judges the weight gradients: the
oracle generator + twin loss evaluated in float64 and in float32 with every LeakyReLU branch forced to the device pass's signs, and

    || dz_HIP - dz_64 ||  <=  3 || dz_32 - dz_64 ||  +  2e-6 || dz_64 ||     per sample,     flips <= max(20, elements // 100000)

(a comparison of complete fp32 and fp64 pipelines would measure branch luck, not arithmetic).  Run with -s for the tables
docs/experiments_projection.md quotes."""
import functools

import pytest
import torch

import projection_ref as ref
from conftest import fixture_params, load_fixture
from helpers import build_flag_nets, build_nets, load_fixture_params, synthetic

import pggan_amd as pg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ops = pg.ops
FACTOR, FLOOR = 3.0, 2e-6
U = 2.0 ** -23


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ the loss kernel
# the issue's five shapes (64 is exactly one tile, 128 is 2x2 tiles, 256 the largest one-pass size), the offset-100 cancellation case,
# and the two sizes whose coarsest cells span tiles of 64 pixels: 512 (level 7: 2x2 tiles) and 1024 (level 8: 4x4 tiles, 16x16 tiles)
LOSS_CASES = [(1, 1, 4, 0.0), (2, 3, 8, 0.0), (3, 2, 64, 0.0), (3, 2, 64, 100.0), (2, 1, 128, 0.0), (1, 4, 256, 0.0), (2, 1, 512, 0.0),
              (1, 2, 1024, 0.0)]


@functools.lru_cache(maxsize=None)
def _loss_case(N, C, r, offset):
    g = torch.Generator().manual_seed(N * 1000 + C * 100 + r)
    img = torch.randn(N, C, r, r, generator=g)
    tgt = torch.randn(N, C, r, r, generator=g) + offset
    L = ref.levels(r)
    mixed = [0.5 + 0.25 * l for l in range(L)]
    if L > 2:
        mixed[1] = 0.0
    out = {'img': img, 'tgt': tgt, 'mixed': mixed}
    for name, w in (('ones', None), ('mixed', mixed)):
        out[name + '_ref'] = ref.pyramid_loss_ref(img, tgt, w)
        out[name + '_bound'] = ref.pyramid_bounds_ref(img, tgt, w)
    return out


@pytest.mark.parametrize('N,C,r,offset', LOSS_CASES)
def test_pyramid_loss_against_the_twin(N, C, r, offset):
    case = _loss_case(N, C, r, offset)
    img, tgt = case['img'].to(DEV), case['tgt'].to(DEV)
    for name, w in (('ones', None), ('mixed', case['mixed'])):
        loss, grad = ops.pyramid_loss(img, tgt, w)
        want_l, want_g = case[name + '_ref']
        bound_l, bound_g = case[name + '_bound']
        el = (loss.cpu().double() - want_l).abs()
        eg = (grad.cpu().double() - want_g).abs()
        print('[%d,%d,%d,%d] offset %g weights %s: loss error / bound %.3f, gradient error / bound %.3f (bound = 2^-23 x the terms)'
              % (N, C, r, r, offset, name, float((el / (U * bound_l)).max()), float((eg / (U * bound_g).clamp_min(1e-300)).max())))
        assert tuple(loss.shape) == (N,) and grad.shape == img.shape
        assert bool((el <= U * bound_l).all())
        assert bool((eg <= U * bound_g).all())
        # two calls give the same bits; the loss-only call gives the loss of the full call
        loss2, grad2 = ops.pyramid_loss(img, tgt, w)
        assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(grad), bits(grad2))
        loss3, none = ops.pyramid_loss(img, tgt, w, want_grad=False)
        assert none is None and torch.equal(bits(loss), bits(loss3))


@pytest.mark.parametrize('N,C,r,offset', LOSS_CASES)
def test_pyramid_loss_exact_properties(N, C, r, offset):
    case = _loss_case(N, C, r, offset)
    img, tgt = case['img'].to(DEV), case['tgt'].to(DEV)
    # identical operands: exact zeros
    loss, grad = ops.pyramid_loss(tgt, tgt)
    assert int(bits(loss).abs().max()) == 0 and int(bits(grad).abs().max()) == 0
    L = ref.levels(r)
    if L == 1:
        loss, grad = ops.pyramid_loss(img, tgt, [0.0])
        assert int(bits(loss).abs().max()) == 0 and int(bits(grad).abs().max()) == 0
        return
    # a zero weight equals the shorter pyramid bit for bit: the coarsest level, and every level from the second
    for full, short in (([1.0] * (L - 1) + [0.0], [1.0] * (L - 1)), ([0.75] + [0.0] * (L - 1), [0.75])):
        la, ga = ops.pyramid_loss(img, tgt, full)
        lb, gb = ops.pyramid_loss(img, tgt, short)
        assert torch.equal(bits(la), bits(lb)) and torch.equal(bits(ga), bits(gb))
    # ... and a level in the middle is removed exactly: the remaining levels are the twin's
    w = [1.0] * L
    w[L // 2] = 0.0
    loss, grad = ops.pyramid_loss(img, tgt, w)
    want_l, want_g = ref.pyramid_loss_ref(case['img'], case['tgt'], w)
    bound_l, bound_g = ref.pyramid_bounds_ref(case['img'], case['tgt'], w)
    assert bool(((loss.cpu().double() - want_l).abs() <= U * bound_l).all())
    assert bool(((grad.cpu().double() - want_g).abs() <= U * bound_g).all())


def test_pyramid_loss_refusals_on_the_device():
    x = torch.zeros(1, 1, 8, 8, device=DEV)
    lib_call = pg._lib.call
    scratch = torch.empty(ops.pyramid_scratch_words(1, 1, 8), device=DEV, dtype=torch.float64)
    loss = torch.empty(1, device=DEV)
    args = lambda **kw: [kw.get('img', x.data_ptr()), x.data_ptr(), None, kw.get('nlev', 0), None, loss.data_ptr(), scratch.data_ptr(),
                         kw.get('bytes', scratch.numel() * 8), 1, kw.get('C', 1), kw.get('r', 8), ops._stream()]
    for kw in (dict(img=None), dict(r=12), dict(r=2), dict(nlev=1), dict(bytes=8), dict(C=0)):
        with pytest.raises(RuntimeError, match='PG_E_ARG'):
            lib_call('pg_pyr_loss_grad', *args(**kw))
    for kw in (dict(r=2048), dict(C=5)):
        with pytest.raises(ops.Unsupported):
            lib_call('pg_pyr_loss_grad', *args(**kw))
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):
        lib_call('pg_pyr_loss_grad', *args(img=x.data_ptr() + 4))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ dz on the pass's own linear piece
def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def _g_signs(ctx):
    """Sign patterns of a G pass in the oracle's call order: block0.c1, block0.c2, then c1, c2 of every block (the saved tensors are
    the PixelNorm outputs: same signs as the LeakyReLU inputs)."""
    out = [_nchw(ctx.y1), _nchw(ctx.y2)]
    for rec in ctx.recs:
        out += [_nchw(rec.a1), _nchw(rec.a2)]
    return out


def _double(params):
    return {k: (v.double() if torch.is_tensor(v) else float(v)) for k, v in params.items()}


def _fixture_net(oracle, name, tag=None):
    meta, data = load_fixture(name)
    c = meta['cfg']
    flags = {}
    if tag is None:
        G, _ = build_nets(meta, DEV)
        load_fixture_params(G, data, 'G')
        gp = fixture_params(data, 'G')
    else:
        case = [k for k in meta['cases'] if k['tag'] == tag][0]
        G, _ = build_flag_nets(meta, case, DEV)
        load_fixture_params(G, data, tag + '/G')
        gp = fixture_params(data, tag + '/G')
        g = case['g']
        flags = dict(normalize_latents=g.get('normalize_latents', True), wscale=g.get('wscale', True),
                     g_pixelnorm=g.get('pixelnorm', True), leakyrelu=g.get('leakyrelu', True))
    cfg = oracle.NetCfg(c['resolution'], c['num_channels'], fmap_base=c['fmap_base'], fmap_decay=c['fmap_decay'], fmap_max=c['fmap_max'],
                        latent_size=c['latent_size'], **flags)
    return G, gp, cfg, c


def _criterion(mine, r32, r64, what):
    """The project's own criterion (tests/test_fp64_adjudicator.py), per sample (row)."""
    mine, r32, r64 = mine.detach().cpu().double(), r32.double(), r64.double()
    for n in range(r64.shape[0]):
        e_hip, e_ref, scale = float((mine[n] - r64[n]).norm()), float((r32[n] - r64[n]).norm()), float(r64[n].norm())
        print('    %s sample %d: |fp64| %.3e   HIP %.2e   fp32 oracle %.2e   (relative)' % (what, n, scale, e_hip / scale, e_ref / scale))
        assert e_hip <= FACTOR * e_ref + FLOOR * scale, (what, n, e_hip / scale, e_ref / scale)


DZ_CASES = ([(name, None, d, a) for name in ('tiny16c1', 'tiny32') for d, a in ((0, 1.0), (1, 0.25), (2, 0.5), (2, 1.0))]
            + [('tiny32', None, 3, 0.5), ('tiny32', None, 3, 1.0)]
            # ReLU, and a generator without PixelNorm / latent normalisation: the sweep's r = None and slope = 0 routes
            + [('flags16', 'relu', 2, 0.5), ('flags16', 'nopn', 2, 0.5), ('flags16', 'nopn', 0, 1.0)])


@pytest.mark.parametrize('name,tag,depth,alpha', DZ_CASES)
def test_dz_on_the_linear_piece_of_the_device_pass(oracle, name, tag, depth, alpha):
    G, gp, cfg, c = _fixture_net(oracle, name, tag)
    G.depth, G.alpha = depth, alpha
    N, r = 6, 4 * 2 ** depth
    targets, z, _, _ = synthetic(11 + depth, N, c['num_channels'], r, c['latent_size'])
    proj = pg.Projector(G)
    loss, dz, img, ctx = proj.loss_and_grad(z.to(DEV), targets.to(DEV), return_context=True)
    signs = _g_signs(ctx)
    l32, dz32, _ = ref.loss_and_dz_ref(oracle, gp, cfg, z, targets, depth, alpha, signs=signs)
    l64, dz64, fs = ref.loss_and_dz_ref(oracle, _double(gp), cfg, z.double(), targets.double(), depth, alpha, signs=signs)
    what = '%s%s depth %d alpha %.2f' % (name, '/' + tag if tag else '', depth, alpha)
    print('%s: %d of %d branches of the device pass differ from those of the fp64 pass' % (what, fs.flips, fs.elements))
    assert fs.flips <= max(20, fs.elements // 100000)
    _criterion(dz, dz32, dz64, what + ' dz')
    assert tuple(dz.shape) == (N, c['latent_size']) and tuple(img.shape) == (N, c['num_channels'], r, r)
    el = (loss.cpu().double() - l64).abs()
    assert bool((el <= FACTOR * (l32.double() - l64).abs() + FLOOR * l64.abs().clamp_min(1.0)).all()), (what, el)


# ------------------------------------------------------------------------------------------------ the search
def test_first_steps_follow_the_twin(oracle):
    """Three Adam steps from the same start: the trajectories of a non-convex problem separate later."""
    G, gp, cfg, c = _fixture_net(oracle, 'tiny16c1')
    depth, alpha, N, steps = 2, 0.5, 4, 3
    G.depth, G.alpha = depth, alpha
    targets, z0, _, _ = synthetic(5, N, 1, 16, c['latent_size'])
    res = pg.Projector(G, steps=steps, lr=0.1).project(targets.to(DEV), z0=z0.to(DEV))
    z32, h32, f32 = ref.project_ref(oracle, gp, cfg, targets, z0, steps, 0.1, (0.9, 0.999), depth, alpha)
    z64, h64, f64 = ref.project_ref(oracle, _double(gp), cfg, targets.double(), z0.double(), steps, 0.1, (0.9, 0.999), depth, alpha)
    assert tuple(res.history.shape) == (steps, N) and tuple(res.z.shape) == (N, c['latent_size']) and tuple(res.images.shape) == (N, 1, 16, 16)
    hist = torch.cat([res.history.cpu().double(), res.loss.cpu().double()[None]])
    want32, want64 = torch.cat([h32.double(), f32.double()[None]]), torch.cat([h64, f64[None]])
    for t in range(steps + 1):
        e_hip, e_ref, scale = float((hist[t] - want64[t]).norm()), float((want32[t] - want64[t]).norm()), float(want64[t].norm())
        print('losses %s: |fp64| %.4e   HIP %.2e   fp32 twin %.2e   (relative)'
              % ('before step %d' % t if t < steps else 'at the end', scale, e_hip / scale, e_ref / scale))
        assert e_hip <= FACTOR * e_ref + FLOOR * scale, (t, e_hip / scale, e_ref / scale)
    _criterion(res.z, z32, z64, 'z after %d steps' % steps)
    assert float((res.z.cpu() - z0).abs().max()) > 0.05                     # (it moved: three steps of lr ~ 0.1)


def test_it_inverts_its_own_images():
    """Targets G(z*) on tiny16c1 at (depth 1, alpha 0.25), lr 0.1, 100 steps from other latents: every sample's final loss is at most a
    quarter of its first.  The float64 twin on the same parameters, targets and start reaches 0.010 .. 0.033 of the first loss
    (docs/experiments_projection.md), inside the 0.08 the cap asks of the twin."""
    meta, data = load_fixture('tiny16c1')
    G, _ = build_nets(meta, DEV)
    load_fixture_params(G, data, 'G')
    G.depth, G.alpha = 1, 0.25
    L = meta['cfg']['latent_size']
    zstar = torch.randn(4, L, generator=torch.Generator().manual_seed(21))
    z0 = torch.randn(4, L, generator=torch.Generator().manual_seed(22))
    targets = G.forward(zstar.to(DEV)).clone()
    res = pg.Projector(G, steps=100, lr=0.1).project(targets, z0=z0.to(DEV))
    first, last = res.history[0].cpu().double(), res.loss.cpu().double()
    print('final / first loss per sample:', ['%.4f' % v for v in (last / first).tolist()])
    assert bool((last <= 0.25 * first).all()), (last / first).tolist()
    assert bool(torch.isfinite(res.history).all())


def test_default_start_is_seeded():
    meta, data = load_fixture('tiny16c1')
    G, _ = build_nets(meta, DEV)
    load_fixture_params(G, data, 'G')
    G.depth, G.alpha = 0, 1.0
    targets = synthetic(1, 2, 1, 4, 32)[0].to(DEV)
    a = pg.Projector(G, steps=1, lr=1e-30, seed=5).project(targets)        # (a step of 1e-30: z stays the start latents)
    b = pg.Projector(G, steps=1, lr=1e-30, seed=5).project(targets)
    c = pg.Projector(G, steps=1, lr=1e-30, seed=6).project(targets)
    assert torch.equal(a.z, b.z) and not torch.equal(a.z, c.z) and tuple(a.z.shape) == (2, 32)


# ------------------------------------------------------------------------------------------------ it touches nothing
def _net_state(G):
    return dict(version=G._param_version, derived=G._rt.derived_ver, bwd=G._rt.bwd_wanted,
                flags=[(m._wt_wanted, m._wino_wanted) for m in G._layers()],
                param=G._flat_param.clone(), grad=G._flat_grad.clone(), wt=G._flat_wt.clone())


def test_a_projection_touches_nothing_of_the_network():
    """A network wide enough that its forward pass runs Winograd layers (64 channels at 16x16 and 32x32 with 8 images), as an evaluation
    copy that has never run a backward sweep.  After one forward pass of its own (which is what derives the forward weights), a
    projection leaves the parameters, the gradient buffer, the version, every layer's request flags and the derived-weight state as
    they were -- in particular it never asks the engine for backward-data copies."""
    torch.manual_seed(3)
    G = pg.Generator((1, 3, 32, 32), fmap_base=512, fmap_max=64, latent_size=64).to(DEV)
    G.depth, G.alpha = 3, 0.5
    targets, z, _, _ = synthetic(2, 8, 3, 32, 64)
    G.forward(z.to(DEV))
    G._flat_grad.normal_()                                                # (something to be left alone)
    before = _net_state(G)
    assert any(w for _, w in before['flags']) and not before['bwd'] and not any(w for w, _ in before['flags'])
    res = pg.Projector(G, steps=3).project(targets.to(DEV))
    torch.cuda.synchronize()
    after = _net_state(G)
    assert after['version'] == before['version'] and after['derived'] == before['derived'] and after['flags'] == before['flags']
    assert after['bwd'] is False
    for k in ('param', 'grad', 'wt'):
        assert torch.equal(bits(after[k]), bits(before[k])), k
    assert all(p.grad is None for p in G.parameters())
    assert bool(torch.isfinite(res.loss).all()) and bool(torch.isfinite(res.history).all())


# ------------------------------------------------------------------------------------------------ it follows the parameters
def test_packed_weights_follow_the_parameters(oracle):
    G, gp, cfg, c = _fixture_net(oracle, 'tiny16c1')
    G.depth, G.alpha = 2, 1.0
    targets, z, _, _ = synthetic(4, 6, 1, 16, c['latent_size'])
    z_d, t_d = z.to(DEV), targets.to(DEV)
    proj = pg.Projector(G)
    proj.loss_and_grad(z_d, t_d)
    first = proj.packed_weights().clone()

    def fresh(net):
        p = pg.Projector(net)
        p.loss_and_grad(z_d, t_d)
        return p.packed_weights()

    def same_as_fresh(net, p, what):
        """The kept projector's copies are those of a new one, bit for bit (the pack is deterministic); its dz, whose small-map convs
        commit K slices with atomics, is judged on the pass's own linear piece with the network's CURRENT parameters."""
        loss, dz, _, ctx = p.loss_and_grad(z_d, t_d, return_context=True)
        assert torch.equal(bits(p.packed_weights()), bits(fresh(net))), what
        params = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in net.reference_state_dict().items()}
        signs = _g_signs(ctx)
        _, dz32, _ = ref.loss_and_dz_ref(oracle, params, cfg, z, targets, int(net.depth), float(net.alpha), signs=signs)
        _, dz64, _ = ref.loss_and_dz_ref(oracle, _double(params), cfg, z.double(), targets.double(), int(net.depth), float(net.alpha), signs=signs)
        _criterion(dz, dz32, dz64, what)

    # load_state_dict (torch-side copy: noticed through _sync_version)
    sd = {k: (v * 1.5 if v.dtype.is_floating_point else v) for k, v in G.state_dict().items()}
    G.load_state_dict(sd)
    same_as_fresh(G, proj, 'load_state_dict')
    assert not torch.equal(bits(proj.packed_weights()), bits(first))
    # a raw-pointer update + mark_params_changed
    second = proj.packed_weights().clone()
    ops.ema(G._flat_param, torch.zeros_like(G._flat_param), 0.5)
    G.mark_params_changed()
    same_as_fresh(G, proj, 'mark_params_changed')
    assert not torch.equal(bits(proj.packed_weights()), bits(second))
    # a smoothed generator's update
    ema = pg.GeneratorEMA(G, beta=0.5)
    ps = pg.Projector(ema.network())
    ps.loss_and_grad(z_d, t_d)
    third = ps.packed_weights().clone()
    ops.ema(G._flat_param, torch.zeros_like(G._flat_param), 0.5)
    G.mark_params_changed()
    ema.update(16)
    same_as_fresh(ema.network(), ps, 'GeneratorEMA.update')
    assert not torch.equal(bits(ps.packed_weights()), bits(third))
    # a change of depth repacks for the live layers of that depth
    G.depth = 1
    t1 = synthetic(4, 6, 1, 8, c['latent_size'])[0].to(DEV)
    proj.loss_and_grad(z_d, t1)
    assert proj.packed_weights().numel() < second.numel()


# ------------------------------------------------------------------------------------------------ the consumers
class _Trainer(object):
    parallel = None
    g_ema = None
    cur_nimg = 7000

    def __init__(self, G):
        self.G = G
        self.stats = {}


def test_monitor_with_a_device_dataset_writes_stats_and_the_sheet(tmp_path):
    """The tail of a DeviceImageDataset at the network's stage, the same targets at every tick, through the real Projector."""
    import os
    meta, data = load_fixture('tiny16c1')
    G, _ = build_nets(meta, DEV)
    load_fixture_params(G, data, 'G')
    G.depth, G.alpha = 2, 1.0
    images = torch.randint(0, 256, (12, 1, 16, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    ds = pg.DeviceImageDataset(images, model_initial_depth=2)
    cursor = ds.cursor
    got = []

    def proc(batch, description):
        got.append((batch, description))
    proc.accepts_device_tensors = True
    m = pg.ProjectionMonitor(ds, num_images=4, steps=5, samples_path=str(tmp_path), resolution=32, postprocessors=[proc], lr=0.05)
    tr = _Trainer(G)
    m.register(tr)
    m.epoch(1)
    first = dict((k, v['val']) for k, v in tr.stats.items())
    m.epoch(2)
    assert set(tr.stats) == {'proj_loss', 'proj_loss_max'} and 0.0 < first['proj_loss'] <= first['proj_loss_max']
    assert ds.cursor == cursor                                                       # the training stream did not move
    want = ops.real_prepare_u8(images[-4:].to(DEV), 1.0)
    for batch, description in got:
        assert description == 'proj_000007' and tuple(batch.shape) == (8, 1, 16, 16)
        assert torch.equal(batch[0::2], want)                                        # the tail, unmirrored, alpha 1: fixed across ticks
    recon = got[0][0][1::2]
    assert bool(torch.isfinite(recon).all()) and not torch.equal(recon, want)
    assert os.path.exists(os.path.join(str(tmp_path), 'proj_000007.png'))


def test_project_samples_is_the_inverse_of_output_samples(tmp_path):
    meta, data = load_fixture('tiny16c1')
    G, _ = build_nets(meta)
    load_fixture_params(G, data, 'G')
    G.depth, G.alpha = 1, 1.0
    path = str(tmp_path / 'generator.dat')
    torch.save(G, path)
    targets = torch.randint(0, 256, (3, 1, 8, 8), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    seen = []

    def dev_proc(batch, description):
        seen.append(('dev', batch, description))
    dev_proc.accepts_device_tensors = True
    z = pg.project_samples(path, targets, [dev_proc, lambda batch, description: seen.append(('host', batch, description))], 'resynth',
                           steps=20, lr=0.1, seed=4)
    assert tuple(z.shape) == (3, 32) and z.is_cuda and bool(torch.isfinite(z).all())
    (_, dev_batch, d1), (_, host_batch, d2) = seen
    assert d1 == d2 == 'resynth' and tuple(dev_batch.shape) == (6, 1, 8, 8) and host_batch.shape == (6, 1, 8, 8)
    t = ops.real_prepare_u8(targets.to(DEV), 1.0)
    assert torch.equal(dev_batch[:3], t) and torch.equal(torch.from_numpy(host_batch), dev_batch.cpu())
    # the reconstructions are the images of the returned latents, and closer to the targets than the start latents' images
    Gd = torch.load(path, weights_only=False).to(DEV)
    recon = Gd.forward(z)
    assert float((recon - dev_batch[3:]).abs().max()) <= 1e-4
    start = pg.utils.device_latents(3, 32, seed=4, device=DEV)()
    l_end, _ = ops.pyramid_loss(dev_batch[3:].contiguous(), t, want_grad=False)
    l_start, _ = ops.pyramid_loss(Gd.forward(start), t, want_grad=False)
    assert bool((l_end < l_start).all())
    # fp32 targets are taken as they are
    z2 = pg.project_samples(path, t.cpu().numpy(), [], 'x', steps=20, lr=0.1, seed=4)
    assert tuple(z2.shape) == (3, 32) and bool(torch.isfinite(z2).all())
    with pytest.raises(ValueError, match='uint8 or float32'):
        pg.project_samples(path, targets.double(), [], 'x')
