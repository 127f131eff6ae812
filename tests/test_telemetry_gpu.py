"""The loss and weight statistics on the device: ``pg_scalar_stats_push`` and ``pg_segment_stats_f32`` / ``pg_segment_stats_finish``
against the fp64 restatement of their definition (tests/telemetry_ref.py: exactly rounded sums, worst-case bounds of any summation
order), and ``LossMonitor`` / ``HealthMonitor`` under a real ``Trainer``, eager and replayed from launch plans.

Shapes: segment lengths 1, 3, 4, 5, chunk - 1, chunk, chunk + 1 and 20000 (tail only, one 16-byte group, group + tail, a chunk less
one, exactly one, one more, several chunks with a ragged last), tables of 1 and of 70 segments in one buffer whose padding is NaN;
sources of 1 (0-dim), 3, 16, 64, 65 and 4096 elements (below, at and above one element per lane; the largest allowed), records of
1, 4 and 8 slots with a skipped one."""
import ctypes
import math

import numpy as np
import pytest
import torch

import telemetry_ref as ref

import pggan_amd as pg

pytestmark = pytest.mark.gpu

DEV = 'cuda'
tel = pg.telemetry
SOURCE_SHAPES = ((), (3,), (16, 1), (64,), (65,), (4096,))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).clone()


@pytest.fixture(scope='module')
def table70():
    """70 segments in one buffer, their device object, and the two seeded host fills: shared, never written."""
    segments, total = ref.layout(70)
    return dict(segments=segments, total=total, seg=tel.SegmentStats(segments, DEV, total),
                ints=ref.fill(total, segments, 'int'), randn=ref.fill(total, segments, 'randn', seed=1))


# ----------------------------------------------------------------------------------------------- segments
def test_segments_integer_data_is_exact(table70):
    t = table70
    got = t['seg'].measure(torch.from_numpy(t['ints']).to(DEV))
    assert got.shape == (70, 4) and got.dtype == torch.float64 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), ref.segment_stats(t['ints'], t['segments']))      # sums, maxabs and counts with ==; NaN padding unread


def test_segments_random_data_within_the_summation_bound_and_reproducible(table70):
    t = table70
    flat = torch.from_numpy(t['randn']).to(DEV)
    first = t['seg'].measure(flat)
    got, want, bound = first.cpu().numpy(), ref.segment_stats(t['randn'], t['segments']), ref.segment_bounds(t['randn'], t['segments'])
    err = np.abs(got[:, :2] - want[:, :2])
    print('segments: max err / bound: sum %.3e, sumsq %.3e' % tuple((err / np.maximum(bound, 1e-300)).max(axis=0)))
    assert np.all(err <= bound)
    assert np.array_equal(got[:, 2:], want[:, 2:])                             # maxabs and the count with ==
    again = t['seg'].measure(flat)
    assert torch.equal(_bits(first), _bits(again))                              # the same input twice: the same bits
    twin = tel.SegmentStats(t['segments'], 'cpu', t['total']).measure(torch.from_numpy(t['randn']))
    assert torch.equal(_bits(first), _bits(twin))                               # the twin sums in the kernel's order


def test_a_segment_does_not_depend_on_the_others(table70):
    t = table70
    flat = torch.from_numpy(t['randn']).to(DEV)
    base = t['seg'].measure(flat).clone()
    for keep in (3, 7, 20, 69):                                                 # lengths 5, 20000, 8191, 8192
        other = torch.full_like(flat, float('nan'))
        other[1::2] = 3.0e38
        off, n = t['segments'][keep]
        other[off:off + n] = flat[off:off + n]
        got = t['seg'].measure(other)
        assert torch.equal(_bits(got[keep]), _bits(base[keep])), keep
        assert int(got[keep + 1 if keep < 69 else 0][3]) > 0                     # (the neighbours really were overwritten)


def test_segments_non_finite_elements_are_counted_and_left_out(table70):
    t = table70
    flat = torch.from_numpy(t['ints']).to(DEV)
    nan, inf = float('nan'), float('inf')
    plant = {}
    for (off, n), where in zip(t['segments'], (0, 2, 1, 4, 4097, ref.CHUNK - 1, ref.CHUNK, 19999)):      # body, group, ragged tails
        plant[off + where] = (nan, inf, -inf)[where % 3]
    off = t['segments'][7][0]                                                   # both sides of a chunk boundary of the 20000 segment
    plant.update({off + ref.CHUNK - 1: inf, off + ref.CHUNK: nan, off + 2 * ref.CHUNK: -inf, off + 2 * ref.CHUNK - 3: nan})
    off = t['segments'][15][0]
    flat[off:off + 20000].fill_(-inf)                                           # a segment without a finite element
    idx = torch.tensor(sorted(plant), device=DEV)
    flat[idx] = torch.tensor([plant[i] for i in sorted(plant)], device=DEV)
    host = flat.cpu().numpy()
    want = ref.segment_stats(host, t['segments'])
    got = t['seg'].measure(flat).cpu().numpy()
    assert np.array_equal(got, want)
    assert want[7, 3] == 5 and want[0, 3] == 1 and tuple(want[15]) == (0.0, 0.0, 0.0, 20000.0) and want[8:15, 3].sum() == 0


def test_table_of_one_segment_and_argument_errors():
    for n in ref.LENGTHS:
        flat = ref.fill(n + 8, [(4, n)], 'int', seed=n)
        got = tel.SegmentStats([(4, n)], DEV, n + 8).measure(torch.from_numpy(flat).to(DEV)).cpu().numpy()
        assert np.array_equal(got, ref.segment_stats(flat, [(4, n)])), n
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):
        tel.SegmentStats([(2, 8)], DEV, 64)
    seg = tel.SegmentStats([(0, 8)], DEV, 64)
    flat = torch.zeros(68, device=DEV)
    with pytest.raises(ValueError):
        seg.measure(flat[:60])
    with pytest.raises(ValueError):
        seg.measure(torch.zeros(64))
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(4, device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):                       # a base that is not 16-byte aligned: nothing is launched
        pg._lib.call('pg_segment_stats_f32', flat.data_ptr() + 4, 64, seg._chunks.data_ptr(), 1, out.data_ptr(), s)


# ----------------------------------------------------------------------------------------------- scalars
def _sources(kind, rng):
    return [np.asarray(rng.randint(-1024, 1025, size=s) if kind == 'int' else rng.standard_normal(s), dtype=np.float32) for s in SOURCE_SHAPES]


@pytest.mark.parametrize('K', [1, 4, 8])
def test_scalar_push_against_the_reference(K):
    rng = np.random.RandomState(K)
    names = ['s%d' % k for k in range(K)]
    skipped = 2 if K > 1 else None                                              # a null slot
    for kind in ('int', 'randn'):
        st = tel.ScalarStats(names)
        want = [list(ref.EMPTY) for _ in names]
        tol, mag = [0.0] * K, [0.0] * K
        for push in range(4):
            pool = _sources(kind, rng)
            host = [None if k == skipped else pool[(k + push) % len(pool)] for k in range(K)]
            st.push(*[None if h is None else torch.from_numpy(h).to(DEV) for h in host])
            for k, h in enumerate(host):
                if h is not None:
                    ref.fold(want[k], ref.source_value(h))
                    tol[k] += ref.value_bound(h)
                    mag[k] += abs(want[k][5])
        assert st.on_device
        rec = st.record()
        for k in range(K):
            if kind == 'int' or k == skipped:
                assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(rec[k].tolist(), want[k])), (kind, k, rec[k], want[k])
            else:
                # counts, first_bad with ==; the values to their bound (header of tests/telemetry_ref.py); their running sum: both sides add
                # the four values in push order, the inputs differ by at most tol, each of the 2 x 3 roundings is at most u x sum|value|
                assert (rec[k][0], rec[k][6], rec[k][7]) == (4.0, 0.0, -1.0)
                assert abs(rec[k][1] - want[k][1]) <= tol[k] + 8 * ref.U * mag[k]
                for f in (3, 4, 5):
                    assert abs(rec[k][f] - want[k][f]) <= tol[k]
        again = tel.ScalarStats(names)                                          # the same pushes of the last round: the same bits
        again.push(*[None if h is None else torch.from_numpy(h).to(DEV) for h in host])
        one = tel.ScalarStats(names)
        one.push(*[None if h is None else torch.from_numpy(h).to(DEV) for h in host])
        assert np.array_equal(again.record().view(np.int64), one.record().view(np.int64))


def test_scalar_non_finite_pushes_reset_and_limits():
    st = tel.ScalarStats(['a', 'b', 'c', 'd'])
    vals = [0.5 * i - 1.0 for i in range(9)]
    for i, v in enumerate(vals):
        a = torch.full((65,), v, device=DEV)
        if i == 5:
            a[64] = float('nan')                                                # in the second element of lane 0
        b = torch.tensor(float('inf') if i >= 7 else v, device=DEV)
        c = torch.full((3, 1), -float('inf') if i == 0 else v, device=DEV)
        st.push(a, b, c, None)
    got = st.read(reset=False)
    others = [v for i, v in enumerate(vals) if i != 5]
    assert (got['a']['first_bad'], got['a']['nonfinite'], got['a']['count']) == (5, 1, 8)
    assert got['a']['mean'] == math.fsum(others) / 8 and got['a']['min'] == -1.0 and got['a']['max'] == 3.0 and got['a']['last'] == 3.0
    assert (got['b']['first_bad'], got['b']['nonfinite'], got['b']['count'], got['b']['last']) == (7, 2, 7, float('inf'))
    assert (got['c']['first_bad'], got['c']['nonfinite'], got['c']['count'], got['c']['min']) == (0, 1, 8, -0.5)
    assert got['d']['count'] == 0 and got['d']['first_bad'] == -1 and math.isnan(got['d']['last'])
    assert st.read()['a'] == got['a']                                           # reset=False had left the record alone
    empty = st.read()                                                           # nothing pushed since the reset
    assert all(r['count'] == 0 and r['nonfinite'] == 0 and r['first_bad'] == -1 and math.isnan(r['last']) for r in empty.values())
    st.push(torch.tensor(2.0, device=DEV), None, None, None)                    # the reset travels with this push
    rec = st.record()
    assert rec[0].tolist() == [1.0, 2.0, 4.0, 2.0, 2.0, 2.0, 0.0, -1.0]
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for k in (1, 2, 3) for a, b in zip(rec[k].tolist(), ref.EMPTY))
    # limits: 4097 elements is PG_E_ARG and launches nothing; the wrapper refuses before the call
    big = torch.zeros(4097, device=DEV)
    record = pg.ops.scalar_stats_record(1, DEV)
    ptrs, lens = (ctypes.c_void_p * 1)(big.data_ptr()), (ctypes.c_int * 1)(4097)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg._lib.call('pg_scalar_stats_push', record.data_ptr(), ptrs, lens, 1, 1, s)
    with pytest.raises(RuntimeError, match='PG_E_ARG'):
        pg._lib.call('pg_scalar_stats_push', record.data_ptr(), ptrs, lens, 9, 1, s)
    with pytest.raises(ValueError):
        pg.ops.scalar_stats_push(record, [big])
    with pytest.raises(ValueError):
        pg.ops.scalar_stats_push(record, [big[:8].double()])
    with pytest.raises(TypeError):
        st.push(1.0, None, None, None)                                          # a device object stays a device object


# ----------------------------------------------------------------------------------------------- under Trainer
SHAPE = (1, 3, 16, 16)
KW = dict(fmap_base=128, fmap_max=32)
LATENT = 32


class _Checker(pg.Plugin):
    """Reads the same four tensors on the host, every iteration (what the reference's monitors do), and keeps the stats of every tick."""

    def __init__(self):
        super(_Checker, self).__init__([(1, 'iteration'), (1, 'epoch')])
        self.values, self.ticks = [], []

    def register(self, trainer):
        self.trainer = trainer

    def iteration(self, i, *losses):
        self.values.append([t.detach().double().cpu().numpy().reshape(-1) for t in losses])

    def epoch(self, tick):
        self.ticks.append({k: dict(v) for k, v in self.trainer.stats.items() if isinstance(v, dict)})


def _trainer(seed=21):
    torch.manual_seed(seed)
    G = pg.Generator(SHAPE, latent_size=LATENT, **KW).to(DEV)
    D = pg.Discriminator(SHAPE, **KW).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def reals():
        while True:
            r = 4 * 2 ** int(G.depth)
            yield torch.rand((4, 3, r, r), device=DEV, generator=gen) * 2 - 1
    opt_g = pg.FusedAdam(G.parameters(), 0.001, betas=(0.0, 0.99))
    opt_d = pg.FusedAdam(D.parameters(), 0.001, betas=(0.0, 0.99))
    tr = pg.Trainer(D, G, pg.wgan_gp_D_loss, pg.wgan_gp_G_loss, opt_d, opt_g, None, reals(),
                    lambda: torch.randn((4, LATENT), device=DEV, generator=gen), tick_nimg_default=16)
    G.depth = D.depth = 1
    return tr


@pytest.mark.parametrize('mode', ['eager', 'plans'])
def test_loss_monitor_under_trainer(mode, monkeypatch):
    """Eight iterations in two ticks of four (minibatch 4, ticks of 16 images).  In plan mode iterations 1-2 warm up, 3 records and
    4-8 replay, so the second tick is made of replayed steps only: their losses are views of one reused buffer."""
    monkeypatch.setattr(pg.wgan_gp_loss, '_use_graphs', False if mode == 'eager' else 'auto')
    monkeypatch.setattr(pg.wgan_gp_loss, '_use_plans', True)
    calls = {}

    def hook(fn, args, name):
        calls[name] = calls.get(name, 0) + 1
        return fn(*args)
    monkeypatch.setattr(pg._lib, 'CALL_HOOK', hook)
    replayed = pg.plans.STATS['replayed']
    tr = _trainer()
    mon, chk, hm = pg.LossMonitor(), _Checker(), pg.HealthMonitor()
    for plugin in (mon, chk, hm):                                               # the checker fires behind the monitor: its read is the later one
        tr.register_plugin(plugin)
    tr.run(total_kimg=0.032)
    assert tr.iterations == 8 and tr.cur_tick == 2 and len(chk.ticks) == 2
    assert calls['pg_scalar_stats_push'] == 8                                   # exactly one library call per iteration
    assert (pg.plans.STATS['replayed'] - replayed >= 10) == (mode == 'plans')   # the issue mode was really taken
    assert mon.scalars.on_device
    for tick in range(2):
        for k, name in enumerate(mon.names):
            series = chk.values[4 * tick:4 * tick + 4]
            vals = [ref.source_value(it[k]) for it in series]
            tol = sum(ref.value_bound(it[k]) for it in series)
            st = chk.ticks[tick][name]
            mean = math.fsum(vals) / 4
            # the mean of four values: their own bounds, four additions and one division on top (tests/telemetry_ref.py)
            bound = tol / 4 + 6 * ref.U * sum(abs(v) for v in vals) / 4
            print('%s tick %d %s: mean %.9g (host %.9g), err %.3e, bound %.3e' % (mode, tick, name, st['val'], mean, abs(st['val'] - mean), bound))
            assert abs(st['val'] - mean) <= bound and st['epoch_mean'] == st['val']
            assert st['count'] == 4 and st['nonfinite'] == 0 and st['first_bad'] == -1
            assert abs(st['last'] - vals[-1]) <= tol and abs(st['min'] - min(vals)) <= tol and abs(st['max'] - max(vals)) <= tol
    assert chk.ticks[0]['D_loss']['val'] != chk.ticks[1]['D_loss']['val']
    # HealthMonitor beside it: norms of the weights and of the last gradients (beta1 = 0) against torch in fp64
    for which, net, opt in (('G', tr.G, tr.optimizer_g), ('D', tr.D, tr.optimizer_d)):
        segs = tel.segments_of(net)
        w, m = net._flat_param.double(), opt.flat_moments(net)[0].double()
        wn = math.sqrt(sum(float(w[o:o + n].pow(2).sum()) for _, o, n in segs))
        gn = math.sqrt(sum(float(m[o:o + n].pow(2).sum()) for _, o, n in segs))
        rel = w.numel() * ref.U                                                 # two fp64 sums of squares in different orders, then a square root
        assert tr.stats[which + '_wnorm']['val'] == pytest.approx(wn, rel=rel) and wn > 1
        assert tr.stats[which + '_gnorm']['val'] == pytest.approx(gn, rel=rel) and gn > 0
        assert tr.stats[which + '_gmax']['val'] == float(m.abs().max())
    # a weight of one layer set to Inf before a tick: the guard names that layer
    tr.D.blocks[1].c2.conv.weight.data.view(-1)[17] = float('inf')
    with pytest.raises(pg.TrainingDiverged) as e:
        hm.epoch(3)
    assert 'D has non-finite values in blocks.1.c2.weight: 1 of' in str(e.value) and 'G has' not in str(e.value) and 'loss' not in str(e.value)
