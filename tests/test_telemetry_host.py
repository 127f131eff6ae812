"""Host side of the loss and weight statistics (no device): the C-ABI declarations, the numpy twin of ``telemetry.ScalarStats`` /
``telemetry.SegmentStats`` against the independent reference (tests/telemetry_ref.py), the library's host-only chunking rule, the
segment table of a network, ``FusedAdam.flat_moments`` and both plugins on a stub trainer.  The kernels are checked on the device
(tests/test_telemetry_gpu.py, tests/test_telemetry_redzone_gpu.py)."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import telemetry_ref as ref

import pggan_amd as pg

tel = pg.telemetry
SHAPE = (1, 3, 16, 16)
KW = dict(fmap_base=128, fmap_max=32)


def test_names_signatures_and_header():
    P, I, L = pg._lib.P, pg._lib.I, pg._lib.L
    sig = pg._lib.SIGNATURES
    assert sig['pg_scalar_stats_push'] == [P, P, P, I, I, P]
    assert sig['pg_segment_stats_plan'] == [P, P, I, L, P, L, P, P]
    assert sig['pg_segment_stats_f32'] == [P, L, P, L, P, P]
    assert sig['pg_segment_stats_finish'] == [P, L, P, I, P, P]
    assert pg._lib.ABI_VERSION == 27                                        # additive: no signature changed
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'pggan_hip.h')).read()
    for name in ('pg_scalar_stats_push', 'pg_segment_stats_plan', 'pg_segment_stats_f32', 'pg_segment_stats_finish'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\);' % name, hdr)
        assert m, name
        args = [a for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
        assert len(args) == len(sig[name]), (name, args)
        for a, t in zip(args, sig[name]):
            assert ('*' in a or 'pg_stream_t' in a) == (t is P), (name, a)
            if t is L:
                assert 'int64_t' in a
    consts = dict(re.findall(r'#define (PG_STATS_\w+|PG_SEG_CHUNK) (\d+)', hdr))
    assert (int(consts['PG_STATS_MAX_SOURCES']), int(consts['PG_STATS_RECORD']), int(consts['PG_STATS_MAX_LENGTH']), int(consts['PG_SEG_CHUNK'])) == \
        (pg.ops.STATS_MAX_SOURCES, pg.ops.STATS_RECORD, pg.ops.STATS_MAX_LENGTH, pg.ops.SEG_CHUNK) == (8, 8, 4096, ref.CHUNK)
    for name in ('LossMonitor', 'HealthMonitor', 'ScalarStats', 'SegmentStats', 'TrainingDiverged'):
        assert name in pg.__all__ and hasattr(pg, name)
    assert pg.plugins.LossMonitor is pg.LossMonitor and tel.RECORD_FIELDS == ref.RECORD_FIELDS


# ----------------------------------------------------------------------------------------------- the twin against the reference
def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize('kind', ['int', 'randn'])
def test_scalar_twin_against_reference(kind):
    rng = np.random.RandomState(3)
    sizes = ((), (3,), (16, 1), (64,), (65,), (4096,))
    names = ['s%d' % i for i in range(len(sizes))] + ['skipped']
    st = tel.ScalarStats(names)
    want = [list(ref.EMPTY) for _ in names]
    tol = np.zeros(len(names))
    for push in range(5):
        vals = [torch.from_numpy(np.asarray(rng.randint(-1024, 1025, size=s) if kind == 'int' else rng.standard_normal(s), dtype=np.float32))
                for s in sizes]
        st.push(*(vals + [None]))
        for k, v in enumerate(vals):
            ref.fold(want[k], ref.source_value(v.numpy()))
            tol[k] += ref.value_bound(v.numpy())
    rec = st.record()
    assert not st.on_device and rec.shape == (7, 8)
    for k in range(len(sizes)):
        if kind == 'int':
            assert all(_same(float(a), float(b)) for a, b in zip(rec[k], want[k])), (k, rec[k], want[k])
        else:
            assert abs(rec[k][1] - want[k][1]) <= tol[k] + 5 * ref.U * abs(want[k][1])
            assert rec[k][0] == 5 and rec[k][6] == 0 and rec[k][7] == -1
    assert all(_same(float(a), b) for a, b in zip(rec[6], ref.EMPTY))          # the skipped slot stays empty
    got = st.read()
    if kind == 'int':
        assert got['s3'] == ref.summary(want[3])
    else:
        assert got['s3'] == pytest.approx(ref.summary(want[3]), rel=1e-12)
    assert all(_same(float(a), b) for row in st.record() for a, b in zip(row, ref.EMPTY))      # reset by the read


def test_scalar_nan_at_push_5_of_9():
    st = tel.ScalarStats(['a', 'b', 'c'])
    vals = [0.5 * i - 1.0 for i in range(9)]
    for i, v in enumerate(vals):
        a = torch.tensor([v, v + 2.0])
        if i == 5:
            a[1] = float('nan')
        st.push(a, float('inf') if i >= 7 else v, torch.tensor(-float('inf')) if i == 0 else torch.tensor(v))
    got = st.read(reset=False)
    others = [v + 1.0 for i, v in enumerate(vals) if i != 5]
    assert got['a']['first_bad'] == 5 and got['a']['nonfinite'] == 1 and got['a']['count'] == 8
    assert got['a']['mean'] == math.fsum(others) / 8 and got['a']['min'] == min(others) and got['a']['max'] == max(others)
    assert got['a']['last'] == vals[8] + 1.0
    assert (got['b']['first_bad'], got['b']['nonfinite'], got['b']['count'], got['b']['last']) == (7, 2, 7, float('inf'))
    assert (got['c']['first_bad'], got['c']['nonfinite'], got['c']['count']) == (0, 1, 8)
    assert got['a']['std'] == pytest.approx(float(np.std(others)), rel=1e-12)
    assert st.read() == got                                                    # reset=False left the record alone
    empty = st.read()
    assert empty['a']['count'] == 0 and empty['a']['first_bad'] == -1 and math.isnan(empty['a']['mean']) and math.isnan(empty['a']['last'])
    assert empty['a']['min'] == float('inf') and empty['a']['max'] == -float('inf')
    with pytest.raises(ValueError):
        st.push(1.0)
    with pytest.raises(ValueError):
        tel.ScalarStats(['n%d' % i for i in range(9)])


@pytest.mark.parametrize('count', [1, 70])
def test_segment_twin_against_reference(count):
    segments, total = ref.layout(count)
    seg = tel.SegmentStats(segments, 'cpu', total)
    flat = ref.fill(total, segments, 'int')
    got = seg.measure(torch.from_numpy(flat)).numpy()
    assert np.array_equal(got, ref.segment_stats(flat, segments))            # integers: every sum exact, NaN padding never read
    flat = ref.fill(total, segments, 'randn', seed=1)
    got, want, bound = seg.measure(torch.from_numpy(flat)).numpy(), ref.segment_stats(flat, segments), ref.segment_bounds(flat, segments)
    assert np.all(np.abs(got[:, :2] - want[:, :2]) <= bound) and np.array_equal(got[:, 2:], want[:, 2:])
    # planted non-finite values: body, chunk boundary, ragged tail
    flat = ref.fill(total, segments, 'int', seed=2)
    for (off, n), where in zip(segments, (0, 2, 1, 4, 4097, ref.CHUNK - 1, ref.CHUNK, 19999)):
        flat[off + where] = (np.nan, np.inf, -np.inf)[where % 3]
    if count > 1:
        off = segments[7][0]
        flat[off + ref.CHUNK - 1], flat[off + ref.CHUNK], flat[off + 2 * ref.CHUNK] = np.inf, np.nan, -np.inf
    got, want = seg.measure(torch.from_numpy(flat)).numpy(), ref.segment_stats(flat, segments)
    assert np.array_equal(got, want) and want[0, 3] == 1 and (count == 1 or want[7, 3] == 4)


def test_chunking_rule_of_the_library_and_of_the_twin():
    segments, total = ref.layout(70)
    chunks, ranges = tel.cut_segments(segments, total)
    lib_chunks, lib_ranges = pg.ops.segment_stats_plan(segments, total)        # host only: no device is touched
    assert lib_chunks.tolist() == [list(c) for c in chunks] and lib_ranges.tolist() == [list(r) for r in ranges]
    assert all(1 <= n <= ref.CHUNK and o % 4 == 0 for o, n in chunks)
    for (off, n), (first, cnt) in zip(segments, ranges):
        mine = chunks[first:first + cnt]
        assert cnt == -(-n // ref.CHUNK) and mine[0][0] == off and sum(c[1] for c in mine) == n
        assert all(a[0] + a[1] == b[0] for a, b in zip(mine, mine[1:]))
    with pytest.raises(RuntimeError, match='PG_E_ALIGN'):
        pg.ops.segment_stats_plan([(0, 8), (10, 4)], 64)
    with pytest.raises(ValueError, match='PG_E_ALIGN'):
        tel.cut_segments([(0, 8), (10, 4)], 64)
    for bad in ([(0, 0)], [(60, 8)], [(-4, 8)]):
        with pytest.raises(RuntimeError, match='PG_E_ARG'):
            pg.ops.segment_stats_plan(bad, 64)
        with pytest.raises(ValueError):
            tel.cut_segments(bad, 64)


# ----------------------------------------------------------------------------------------------- networks and the optimizer
@pytest.fixture(scope='module')
def nets():
    torch.manual_seed(4)
    return pg.Generator(SHAPE, latent_size=32, **KW), pg.Discriminator(SHAPE, **KW)


def test_segments_cover_every_parameter_once(nets):
    for net in nets:
        segs = tel.segments_of(net)
        params = dict(net.named_parameters())
        assert len(segs) == len(params) == len(set(s[0] for s in segs))
        assert sum(n for _, _, n in segs) == sum(p.numel() for p in params.values())
        assert all(off % 4 == 0 and n >= 1 for _, off, n in segs)
        spans = sorted((off, off + n) for _, off, n in segs)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= net._flat_param.numel()
        base = net._flat_param.data_ptr()
        for name, off, n in segs:                                              # 'blocks.0.c1.weight' is the parameter 'blocks.0.c1.conv.weight'
            p = params[name] if name in params else params[name.rsplit('.', 1)[0] + '.conv.' + name.rsplit('.', 1)[1]]
            assert p.data_ptr() == base + 4 * off and p.numel() == n
    names = [s[0] for s in tel.segments_of(nets[1])]
    assert 'linear.weight' in names and 'linear.bias' in names and 'blocks.0.c1.weight' in names
    assert dict((s[0], s[2]) for s in tel.segments_of(nets[1]))['linear.bias'] == 1


def test_flat_moments_is_none_before_the_first_step(nets):
    G = nets[0]
    opt = pg.FusedAdam(G.parameters(), 0.001, betas=(0.0, 0.99))
    assert opt.flat_moments(G) is None and opt.flat_moments(object()) is None
    base, m, v = opt._new_flat_state(0, opt.param_groups[0], G._flat_param.data_ptr())      # what the first step creates
    got = opt.flat_moments(G)
    assert got[0] is m and got[1] is v and m.numel() == G._flat_param.numel()
    assert opt.flat_moments(nets[1]) is None


# ----------------------------------------------------------------------------------------------- plugins on a stub trainer
class _Opt(object):
    def __init__(self, moments=None):
        self.moments = moments

    def flat_moments(self, net):
        return self.moments


class _Trainer(object):
    def __init__(self, G=None, D=None, opt_g=None, opt_d=None, parallel=None):
        self.G, self.D, self.optimizer_g, self.optimizer_d = G, D, opt_g, opt_d
        self.parallel, self.stats, self.cur_nimg = parallel, {}, 12345


def test_loss_monitor_on_a_stub_trainer():
    mon = pg.LossMonitor()
    assert mon.trigger_interval == [(1, 'iteration'), (1, 'epoch'), (1, 'end')]
    assert mon.names == ('G_loss', 'D_loss', 'D_real', 'D_fake')
    tr = _Trainer()
    mon.register(tr)
    assert tr.loss_monitor is mon and sorted(tr.stats) == ['D_fake', 'D_loss', 'D_real', 'G_loss']
    for tick in (1, 2):
        series = []
        for i in range(4):
            g, d = 0.25 * i + tick, -1.5 * i
            real, fake = torch.tensor([[1.0 + i], [3.0 + i]]), torch.tensor([[float(tick)], [2.0]])
            series.append((g, d, 2.0 + i, 0.5 * tick + 1.0))
            mon.iteration(i + 1, torch.tensor(g), torch.tensor(d), real, fake)
        mon.epoch(tick)
        for k, name in enumerate(mon.names):
            st = tr.stats[name]
            col = [s[k] for s in series]
            assert st['log_name'] == name and st['log_epoch_fields'] == ['{val:.4f}']
            assert st['val'] == st['epoch_mean'] == sum(col) / 4 and st['last'] == col[-1]          # the tick alone: reset at every tick
            assert st['min'] == min(col) and st['max'] == max(col) and st['count'] == 4 and st['nonfinite'] == 0 and st['first_bad'] == -1
            assert st['std'] == pytest.approx(float(np.std(col)), abs=1e-12)
            assert st['log_epoch_fields'][0].format(**st) == '%.4f' % st['val']
    assert mon.last[0] == 2
    before = dict(tr.stats['G_loss'])
    mon.end(1)                                                                 # nothing gathered since the tick closed: no report
    assert tr.stats['G_loss'] == before
    mon.iteration(9, 1.0, 2.0, 3.0, 4.0)
    mon.end(1)
    assert tr.stats['D_fake']['val'] == 4.0 and tr.stats['D_fake']['count'] == 1
    with pytest.raises(ValueError):
        mon.iteration(10, 1.0)


def test_health_monitor_on_a_stub_trainer(nets):
    G, D = nets
    m = torch.zeros_like(G._flat_param)
    name, off, n = [s for s in tel.segments_of(G) if s[0] == 'block0.c2.weight'][0]
    m[off:off + n] = 0.5
    m[off + 3] = -2.0
    tr = _Trainer(G, D, _Opt((m, None)), torch.optim.Adam(D.parameters()))
    hm = pg.HealthMonitor(health_ticks=3, per_layer=True)
    assert hm.trigger_interval == [(3, 'epoch'), (1, 'end')]
    hm.register(tr)
    hm.epoch(3)
    for which, net in (('G', G), ('D', D)):
        want = math.sqrt(sum(float(p.detach().double().pow(2).sum()) for p in net.parameters()))
        st = tr.stats[which + '_wnorm']
        assert st['log_name'] == which + '_wnorm' and st['val'] == pytest.approx(want, rel=1e-12)
    assert tr.stats['G_gnorm']['val'] == pytest.approx(math.sqrt(0.25 * (n - 1) + 4.0), rel=1e-12) and tr.stats['G_gmax']['val'] == 2.0
    assert 'D_gnorm' not in tr.stats and 'D_gmax' not in tr.stats             # a torch.optim optimizer: weights only
    assert tr.stats['G_gnorm/block0.c2.weight']['val'] == tr.stats['G_gnorm']['val'] and 'D_wnorm/linear.bias' in tr.stats
    table = hm.report()
    assert len(table) == len(tel.segments_of(G)) + len(tel.segments_of(D))
    row = [r for r in table if r['net'] == 'G' and r['layer'] == name][0]
    assert (row['offset'], row['length'], row['gmax'], row['w_nonfinite'], row['g_nonfinite']) == (off, n, 2.0, 0, 0)
    assert [r for r in table if r['net'] == 'D'][0]['gnorm'] is None

    # a poisoned layer, a poisoned moment and a poisoned loss
    w = D.blocks[1].c1.conv.weight
    saved = w.data.clone()
    try:
        w.data.view(-1)[5] = float('inf')
        w.data.view(-1)[11] = float('nan')
        m[off + 1] = float('nan')
        lm = pg.LossMonitor()
        lm.register(tr)
        for i in range(4):
            lm.iteration(i + 1, 1.0, float('nan') if i >= 2 else 0.0, 2.0, 3.0)
        with pytest.raises(pg.TrainingDiverged) as e:
            hm.epoch(6)
        msg = str(e.value)
        assert 'blocks.1.c1.weight: 2 of %d weights' % w.numel() in msg and 'block0.c2.weight: 1 of %d first-moment' % n in msg
        assert 'D_loss' in msg and 'first_bad = 2' in msg and '12.345 kimg' in msg and 'G has' in msg and 'D has' in msg
        assert 'blocks.0.c1' not in msg and 'G_loss' not in msg
        lm.epoch(7)                                                            # the loss monitor fired first in this tick: its report is used
        with pytest.raises(pg.TrainingDiverged, match='first_bad = 2'):
            hm.epoch(7)
        soft = pg.HealthMonitor(on_nonfinite='warn')
        soft.register(tr)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            soft.epoch(8)
        assert len(caught) == 1 and issubclass(caught[0].category, RuntimeWarning) and 'blocks.1.c1.weight' in str(caught[0].message)
    finally:
        w.data.copy_(saved)
    m[off + 1] = 0.5
    del tr.loss_monitor
    hm.epoch(9)                                                                # healthy again: no error
    off_rank = _Trainer(G, D, _Opt(), _Opt(), parallel=type('P', (), {'rank': 1})())
    hm2 = pg.HealthMonitor()
    hm2.register(off_rank)
    hm2.epoch(1)
    assert off_rank.stats == {} and hm2.report() == []
    with pytest.raises(ValueError):
        pg.HealthMonitor(on_nonfinite='ignore')
