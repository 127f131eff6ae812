"""The statistics kernels between guard bands (tests/redzone.py, docs/experiments_redzone.md) at the ragged shapes of
tests/test_telemetry_gpu.py: the flat buffer, the chunk table, the segment ranges and the scalar sources are guarded inputs (NaN bands:
a load from outside poisons a sum), partials, result and record are guarded outputs filled with the sentinel.  No band is touched,
no input is changed, every output element is written -- and the results are still the reference's."""
import math

import numpy as np
import pytest
import torch

import telemetry_ref as ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
ops = pg.ops


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    monkeypatch.setattr(ops, 'torch', r.proxy(helpers=(ops._empty, ops.Arena.take)))
    yield r
    r.forget()


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


@pytest.mark.parametrize('n', ref.LENGTHS)
def test_one_segment_fills_the_buffer(rz, n):
    """The segment IS the payload: its first float is the payload's first, its last the payload's last (a [3] bias gets no slack)."""
    flat = ref.fill(n, [(0, n)], 'int', seed=n)
    chunks, ranges = ops.segment_stats_plan([(0, n)], n)
    flat_d = rz.guard(torch.from_numpy(flat), name='flat')
    chunks_d, ranges_d = rz.guard(chunks, name='chunks'), rz.guard(ranges, name='ranges')
    assert flat_d.data_ptr() % 32 == 16
    got = ops.segment_stats(flat_d, chunks_d, ranges_d)
    chk(rz)                                                    # bands intact, inputs unchanged, every partial and every result written
    assert np.array_equal(got.cpu().numpy(), ref.segment_stats(flat, [(0, n)]))


def test_table_of_70_segments(rz):
    segments, total = ref.layout(70)
    segments = [(off - 4, n) for off, n in segments]           # the first segment starts at the payload's first float
    total = segments[-1][0] + segments[-1][1]                  # ... and the last one (8192 floats) ends at its last
    flat = ref.fill(total, segments, 'int', seed=5)
    chunks, ranges = ops.segment_stats_plan(segments, total)
    flat_d = rz.guard(torch.from_numpy(flat), name='flat')
    got = ops.segment_stats(flat_d, rz.guard(chunks, name='chunks'), rz.guard(ranges, name='ranges'))
    chk(rz)
    assert np.array_equal(got.cpu().numpy(), ref.segment_stats(flat, segments))


@pytest.mark.parametrize('K', [1, 4, 8])
def test_scalar_push(rz, K):
    rng = np.random.RandomState(K)
    shapes = ((), (3,), (16, 1), (64,), (65,), (4096,), (5,), (1,))
    host = [np.asarray(rng.randint(-1024, 1025, size=shapes[k]), dtype=np.float32) for k in range(K)]
    if K > 1:
        host[1] = None                                         # a null slot
    srcs = [None if h is None else rz.guard(torch.from_numpy(h), name='source%d' % k) for k, h in enumerate(host)]
    record = ops.scalar_stats_record(K, 'cuda')                # a guarded output: the sentinel everywhere
    ops.scalar_stats_push(record, srcs, reset=True)
    chk(rz)                                                    # the reset writes all K x 8 doubles, skipped slot included
    want = [ref.fold(list(ref.EMPTY), ref.source_value(h)) if h is not None else list(ref.EMPTY) for h in host]
    first = record.cpu().numpy()
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for k in range(K) for a, b in zip(first[k].tolist(), want[k]))
    again = rz.guard(record, name='record', inplace=True)      # a running record: read and written
    ops.scalar_stats_push(again, srcs, reset=False)
    chk(rz)
    for k, h in enumerate(host):
        if h is not None:
            ref.fold(want[k], ref.source_value(h))
    second = again.cpu().numpy()
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for k in range(K) for a, b in zip(second[k].tolist(), want[k]))
