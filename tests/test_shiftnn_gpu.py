"""The shift-invariant window search on the MI355X (csrc/shift_search.hip through ops.shift_l2min_u8, metrics.ShiftNearestNeighbours)
against the product's numpy twin (metrics._shift_keys_host) and the brute force of tests/shiftnn_ref.py.  Integer arithmetic: EVERY
comparison is ``==``, there is no tolerance anywhere.

Shapes are the smallest at which each part can go wrong.  S = 4 and 16 take the plain integer kernel, S = 32 and 64 the MFMA kernel
(8 and 4 rows of a window per step); S = 256 is the first size whose rows are one step each and, with C = 3, the smallest contraction
past the 131072 terms an int32 accumulator holds.  A strip of T = S columns has one start, T = S + 1 two, T = S + 37 a ragged count
whose pitch is no multiple of 16 away; T = S + 300 takes three 128-start workgroups.  The query counts are one MFMA tile, two tiles, a
full launch and two launches."""
import numpy as np
import pytest
import torch

import shiftnn_ref

pytestmark = pytest.mark.gpu

KS = [1, 33, 64, 65]


@pytest.fixture(scope='module')
def pg():
    import pggan_amd
    return pggan_amd


def pack(pg, strips):
    return pg.dataset.StripLevel.pack(strips, 'cuda')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def keys_of(pg, level, q, seg):
    return pg.ops.shift_l2min_u8(level, dev(q), seg).cpu().numpy()


def three_strips(C, S, seed):
    """T = S (one start), T = S + 1, and a T that is not a multiple of 16."""
    return shiftnn_ref.strips([S, S + 1, S + 37], C, S, seed)


# --------------------------------------------------------------------------------------------------- kernel == twin == reference
@pytest.mark.parametrize('S', [4, 16, 32, 64])
@pytest.mark.parametrize('C', [1, 2, 3])
def test_kernel_equals_twin_equals_reference(pg, S, C):
    strips = three_strips(C, S, seed=100 + 10 * S + C)
    q = shiftnn_ref.queries(max(KS), C, S, seed=200 + 10 * S + C)
    q[0] = strips[2][:, :, 7:7 + S]
    level = pack(pg, strips)
    T = S + 37
    for seg in (1, 3, S, 2 * T):
        want = shiftnn_ref.keys(strips, q, seg)                              # [65, G]: the rows of fewer queries are its first rows
        assert np.array_equal(pg.metrics._shift_keys_host(strips, q, seg), want)
        assert want.shape[1] == len(pg.ops.shift_segments([S, S + 1, T], S, seg)[0])
        for K in KS:
            got = keys_of(pg, level, q[:K], seg)
            assert got.dtype == np.int64 and got.shape == (K, want.shape[1])
            assert np.array_equal(got, want[:K]), (S, C, seg, K)
    assert np.array_equal(keys_of(pg, level, q[:2], None), shiftnn_ref.keys(strips, q[:2], S))     # the default segment is S


@pytest.mark.parametrize('S', [4, 32])
def test_several_workgroups_per_strip(pg, S):
    """Three tiles of 128 starts in the second strip; seg = 128 keeps a tile in one segment (the shuffle reduction), seg = 100 and 7
    cut tiles (one atomic per start), seg = 1000 spans all tiles of a strip (tiles combine in one key)."""
    strips = shiftnn_ref.strips([S + 130, S + 300], 2, S, seed=300 + S)
    q = shiftnn_ref.queries(3, 2, S, seed=301 + S)
    q[1] = strips[1][:, :, 257:257 + S]
    level = pack(pg, strips)
    for seg in (128, 100, 7, 1000):
        want = shiftnn_ref.keys(strips, q, seg)
        assert np.array_equal(pg.metrics._shift_keys_host(strips, q, seg), want)
        assert np.array_equal(keys_of(pg, level, q, seg), want), seg
    g = len(pg.ops.shift_segments([S + 130], S, 128)[0]) + 257 // 128
    assert shiftnn_ref.keys(strips, q, 128)[1, g] == 257 % 128              # distance 0 at start 257


# ------------------------------------------------------------------------------------------------------------- planted copy
@pytest.mark.parametrize('S', [16, 64])
def test_planted_copy_is_found_at_its_odd_start(pg, S):
    strips = shiftnn_ref.strips([S + 20, S + 90, S + 5], 2, S, seed=400 + S)
    m, u = 1, 53
    q = shiftnn_ref.queries(2, 2, S, seed=401)
    q[1] = strips[m][:, :, u:u + S]
    nn = pg.metrics.ShiftNearestNeighbours(pack(pg, strips), k=2)
    res = nn.search(dev(pg.dataset.prepare_host(q, 1.0, (0, 255), (-1, 1))))
    assert (int(res['strip'][1, 0]), int(res['start'][1, 0]), int(res['sqdist'][1, 0])) == (m, u, 0) and float(res['rms'][1, 0]) == 0.0
    strip, start, sq = shiftnn_ref.search(strips, q, S, 2)
    assert np.array_equal(res['strip'].numpy(), strip) and np.array_equal(res['start'].numpy(), start) and np.array_equal(res['sqdist'].numpy(), sq)
    assert res['sqdist'][0, 0] > 0 and not res['mirrored'].any()


# --------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize('S', [8, 32])
def test_ties_go_to_the_lower_start_and_the_lower_segment(pg, S):
    period = 5
    base = shiftnn_ref.strips([period], 1, S, seed=500 + S)[0]
    strip = np.tile(base, (1, 1, 40))[:, :, :S + 150]                        # periodic in time: the window at u recurs at u + 5
    q = strip[None, :, :, 3:3 + S].copy()
    level = pack(pg, [strip])
    # one segment: starts 3, 8, 13 ... all match; the lower start wins
    key = keys_of(pg, level, q, 1000)
    assert key.tolist() == [[3]]
    # segments of 20 starts: every segment holds the window (20 = 4 periods); start 3 of each, and the top-k lists the lower segments first
    nn = pg.metrics.ShiftNearestNeighbours(level, k=4, seg=20)
    res = nn.search(dev(pg.dataset.prepare_host(q, 1.0, (0, 255), (-1, 1))))
    assert res['sqdist'].tolist() == [[0, 0, 0, 0]] and res['start'].tolist() == [[0 + 3, 20 + 3, 40 + 3, 60 + 3]]
    want = shiftnn_ref.keys([strip], q, 20)
    assert np.array_equal(keys_of(pg, level, q, 20), want)


# ----------------------------------------------------------------------------------------------------------------- widening
def test_widening_past_the_int32_accumulator(pg):
    """C = 3, S = 256: 196608 terms.  All-255 against all-0 is 65025 * 196608 = 12 784 435 200 > 2^31, and in the shifted domain the
    cross term is 127 * -128 * 196608 < -2^31: an accumulator that is not widened fails."""
    C, S, T = 3, 256, 256 + 5
    hi, lo = np.full((C, S, T), 255, dtype=np.uint8), np.zeros((C, S, T), dtype=np.uint8)
    exact = 65025 * C * S * S
    assert exact > 2 ** 31
    for strip, q in ((hi, lo), (lo, hi)):
        key = keys_of(pg, pack(pg, [strip]), q[None, :, :, :S], S)
        assert key.tolist() == [[exact << 16]]                               # every start ties: the first wins
    # and against the twin on random bytes of that size (the brute force would need 6 starts x 196608 int64: cheap enough too)
    strips = shiftnn_ref.strips([T], C, S, seed=600)
    q = shiftnn_ref.queries(2, C, S, seed=601)
    want = shiftnn_ref.keys(strips, q, 4)
    assert np.array_equal(pg.metrics._shift_keys_host(strips, q, 4), want)
    assert np.array_equal(keys_of(pg, pack(pg, strips), q, 4), want)


# --------------------------------------------------------------------------------------------------- padding and neighbours
@pytest.mark.parametrize('S', [4, 32])
def test_padding_bytes_and_neighbouring_strips_never_reach_a_result(pg, S):
    C = 2
    cols = [S + 37, S, S + 1, S + 21]
    strips = shiftnn_ref.strips(cols, C, S, seed=700 + S)
    q = shiftnn_ref.queries(3, C, S, seed=701 + S)
    clean = pack(pg, strips)
    rows, total = pg.dataset.StripLevel.layout(C, S, cols)
    assert total == clean.buffer.numel()                                     # packed back to back: a strip ends where the next begins
    noisy_buf = torch.from_numpy(np.random.RandomState(7).randint(1, 256, size=total).astype(np.uint8)).cuda()
    noisy = pg.dataset.StripLevel(noisy_buf, clean.table.clone(), C, S, cols)
    for m, s in enumerate(strips):
        noisy.strip(m).copy_(torch.from_numpy(s))
    pad = sum(C * S * (pitch - c) for _, pitch, c in rows)
    assert pad > 0 and int((noisy.buffer != clean.buffer).sum()) > pad // 2  # the padding really differs
    for seg in (1, S):
        want = shiftnn_ref.keys(strips, q, seg)
        assert np.array_equal(keys_of(pg, clean, q, seg), want)
        assert np.array_equal(keys_of(pg, noisy, q, seg), want)
    # the last start of every strip
    last = shiftnn_ref.keys(strips, q, 1)[:, np.cumsum([c - S + 1 for c in cols]) - 1]
    for i, (s, c) in enumerate(zip(strips, cols)):
        assert np.array_equal(last[:, i] >> 16, shiftnn_ref.distances(s, q)[:, c - S])


# ---------------------------------------------------------------------------------------------------------- reproducibility
def test_two_runs_give_the_same_bits(pg):
    S = 32
    strips = shiftnn_ref.strips([S + 300, S + 131], 1, S, seed=800)
    level, q = pack(pg, strips), dev(shiftnn_ref.queries(40, 1, S, seed=801))
    for seg in (1000, 50):                                                   # tiles that share a key through the atomic minimum
        a, b = pg.ops.shift_l2min_u8(level, q, seg), pg.ops.shift_l2min_u8(level, q, seg)
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_a_training_window_off_the_grid_is_a_copy(pg):
    """The test that fails without the feature: a 'generated' sample that IS a training window at a start that is no multiple of R.
    ``NearestNeighbours`` on ``level_stack()`` does not see it; the shift search returns distance 0 at its strip and start."""
    R, C = 64, 2
    strips = shiftnn_ref.strips([R * 4 + 9, R * 3], C, R, seed=900)
    ds = pg.DeviceStripDataset(strips, model_initial_depth=4, pyramid='chain', device='cuda')          # depth 6: the source stage
    direct = pg.DeviceStripDataset(strips, model_initial_depth=4, pyramid='direct', device='cuda')
    for depth, t in ((4, 77), (3, 2 * 45)):                                  # the source stage; one below, shift 1 (t even, t >> 1 odd)
        ds.model_depth = direct.model_depth = depth
        level, shift, dd = ds._stage()
        assert shift == 4 - depth and dd == 0
        idx, pos = torch.tensor([1], device='cuda'), torch.tensor([t], device='cuda')
        sample = pg.ops.crop_batch_u8(level, idx, pos, None, shift, 0, 1.0, (0, 255), (-1, 1))
        other = torch.rand(1, C, R >> shift, R >> shift, device='cuda') * 2 - 1
        samples = torch.cat([sample, other])
        nn = pg.metrics.ShiftNearestNeighbours(ds, k=3)
        res = nn.search(samples)
        assert (int(res['strip'][0, 0]), int(res['start'][0, 0]), int(res['sqdist'][0, 0])) == (1, t, 0)
        assert all(int(s) % (1 << shift) == 0 for s in res['start'].reshape(-1))
        plain = pg.metrics.NearestNeighbours(ds, k=1).search(samples)
        assert int(plain['sqdist'][0, 0]) > 0
        assert bool((res['sqdist'][:, 0] <= plain['sqdist'][:, 0]).all())
        near = nn.neighbours(res)
        want = pg.ops.crop_batch_u8(level, res['strip'].reshape(-1).cuda(), res['start'].reshape(-1).cuda(), None, shift, 0, 1.0,
                                    (0, 255), (-1, 1))
        assert torch.equal(near.reshape(want.shape), want) and torch.equal(near[0, 0], sample[0])
        # the host twin of the whole search
        host = pg.metrics.ShiftNearestNeighbours(ds, k=3, device='cpu').search(samples.cpu())
        for name in ('strip', 'start', 'sqdist', 'rms', 'mirrored'):
            assert torch.equal(res[name], host[name]), name
        # 'direct': the same keys as the level made by pyramid_level_u8
        nd = pg.metrics.ShiftNearestNeighbours(direct, k=3)
        made, scale = nd.level()
        assert scale == shift and made.S == R >> shift
        full = direct._stage()[0]
        by_hand = pack(pg, [pg.ops.pyramid_level_u8(full.strip(m), shift, (0, 255)) for m in range(2)]) if shift else full
        q = pg.ops.quantize_u8(samples)
        assert torch.equal(pg.ops.shift_l2min_u8(made, q), pg.ops.shift_l2min_u8(by_hand, q))
        rd = nd.search(samples)
        if shift <= 1:                                                       # (the two pyramids agree down to one level below the source)
            for name in ('strip', 'start', 'sqdist'):
                assert torch.equal(rd[name], res[name]), name
        assert nd.level()[0] is made                                         # kept until the stage moves


def test_mirror_and_more_queries_than_a_pass(pg):
    S, C = 32, 1
    strips = shiftnn_ref.strips([S + 70, S + 3], C, S, seed=950)
    q = shiftnn_ref.queries(40, C, S, seed=951)                              # mirrored: 80 queries, two passes
    q[5] = strips[0][:, :, 41:41 + S][..., ::-1]
    samples = dev(pg.dataset.prepare_host(q, 1.0, (0, 255), (-1, 1)))
    level = pack(pg, strips)
    res = pg.metrics.ShiftNearestNeighbours(level, k=2, mirror=True, seg=16).search(samples)
    assert (int(res['strip'][5, 0]), int(res['start'][5, 0]), int(res['sqdist'][5, 0]), bool(res['mirrored'][5, 0])) == (0, 41, 0, True)
    host = pg.metrics.ShiftNearestNeighbours(level, k=2, mirror=True, seg=16, device='cpu').search(samples.cpu())
    for name in ('strip', 'start', 'sqdist', 'rms', 'mirrored'):
        assert torch.equal(res[name], host[name]), name


# ------------------------------------------------------------------------------------------------- the entry point's own checks
def test_entry_point_refuses_bad_arguments_before_it_launches(pg):
    S, C = 32, 1
    strips = shiftnn_ref.strips([S + 3], C, S, seed=990)
    level, q = pack(pg, strips), dev(shiftnn_ref.queries(2, C, S, seed=991))
    segtab = pg.ops.shift_table(level, S)
    key = torch.full((2, 1), -7, dtype=torch.int64, device='cuda')
    stream = pg.ops._stream()

    def call(src=None, C=C, S=S, queries=None, K=2, seg=S, out=None):
        pg._lib.call('pg_shift_l2min_u8', level.buffer.data_ptr() if src is None else src, level.table.data_ptr(), 1, C, S,
                     q.data_ptr() if queries is None else queries, K, seg, segtab.data_ptr(), 1, 1, key.data_ptr() if out is None else out, stream)

    for bad in (dict(C=0), dict(C=4), dict(S=2), dict(S=48), dict(S=2048), dict(seg=0), dict(seg=(1 << 16) + 1), dict(K=0), dict(K=65)):
        with pytest.raises(RuntimeError, match='PG_E_ARG'):
            call(**bad)
    for bad in (dict(src=level.buffer.data_ptr() + 8), dict(queries=q.data_ptr() + 4), dict(out=key.data_ptr() + 4)):
        with pytest.raises(RuntimeError, match='PG_E_ALIGN'):
            call(**bad)
    assert key.tolist() == [[-7], [-7]]                                      # nothing was launched
    call()
    assert np.array_equal(key.cpu().numpy(), shiftnn_ref.keys(strips, q.cpu().numpy(), S))
