"""Statistics of the training process itself: the losses of every iteration and the per-layer norms of a network's weights and Adam
moments, taken on the device without a host synchronisation per iteration (csrc/telemetry.hip; definition: DESIGN.md §7, restated in
tests/telemetry_ref.py).

``ScalarStats``   a running record {count, sum, sumsq, min, max, last, non-finite count, first bad push} per name; ``push`` is one launch
                  on the current stream, ``read`` one device-to-host copy of K x 64 bytes.
``SegmentStats``  {sum, sumsq, maxabs, non-finite count} of every (offset, length) segment of a flat fp32 buffer: two launches.

Both take CPU tensors as well and then evaluate a numpy twin of the same definition in the same order of summation (the
``device='cpu'`` convention of ``metrics.NearestNeighbours``): the host tests and users without the library run on it.  A device
tensor never goes through the twin: without the library that is an error, not a slow path."""
import math

import numpy as np
import torch

from . import ops

RECORD_FIELDS = ('n_finite', 'sum', 'sumsq', 'min', 'max', 'last', 'n_nonfinite', 'first_bad')
SEGMENT_FIELDS = ('sum', 'sumsq', 'maxabs', 'n_nonfinite')
_EMPTY = (0.0, 0.0, 0.0, float('inf'), float('-inf'), float('nan'), 0.0, -1.0)


class TrainingDiverged(RuntimeError):
    """A parameter, an Adam moment or a loss of the run is NaN or infinite (``plugins.HealthMonitor``)."""


# ----------------------------------------------------------------------------------------------- numpy twin
def _lane_tree(acc):
    """64 running sums -> one, as the lanes of a wave combine: strides 32, 16, 8, 4, 2, 1, sum i += sum i + stride."""
    acc = acc.copy()
    off = 32
    while off:
        acc[:off] += acc[off:2 * off]
        off >>= 1
    return acc[0]


def _mean_host(x):
    """The value of a source (include/pggan_hip.h, pg_scalar_stats_push): 64 strided running sums in fp64, the lane tree, / n."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    rows = -(-n // 64)
    padded = np.zeros(rows * 64)
    padded[:n] = x
    acc = np.zeros(64)
    with np.errstate(all='ignore'):
        for row in padded.reshape(rows, 64):
            acc += row
        return _lane_tree(acc) / float(n)


def _fold_host(rec, value):
    if math.isfinite(value):
        rec[0] += 1.0
        rec[1] += value
        rec[2] += value * value
        rec[3] = min(rec[3], value)
        rec[4] = max(rec[4], value)
    else:
        if rec[7] < 0.0:
            rec[7] = rec[0] + rec[6]
        rec[6] += 1.0
    rec[5] = value


def _chunk_host(x):
    """One chunk of at most SEG_CHUNK floats -> its partial, in the order of segment_stats_kernel: thread t of 256 takes the groups
    of four t, t + 256, ..., component by component; (c0 + c1) + (c2 + c3); the up to three last elements go to threads 0, 1, 2; the
    lane tree per wave; (w0 + w1) + (w2 + w3)."""
    n = x.size
    ok = np.isfinite(x)
    d = np.where(ok, x, np.float32(0)).astype(np.float64)
    nvec = n // 4
    passes = max(1, -(-nvec // 256))
    body = np.zeros(passes * 256 * 4)
    body[:4 * nvec] = d[:4 * nvec]
    body = body.reshape(passes, 256, 4)
    s, q = np.zeros((256, 4)), np.zeros((256, 4))
    for p in range(passes):
        s += body[p]
        q += body[p] * body[p]
    s = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    q = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
    tail = d[4 * nvec:]
    s[:tail.size] += tail
    q[:tail.size] += tail * tail
    ws = [_lane_tree(s[w * 64:(w + 1) * 64]) for w in range(4)]
    wq = [_lane_tree(q[w * 64:(w + 1) * 64]) for w in range(4)]
    maxabs = float(np.abs(x[ok]).max()) if ok.any() else 0.0
    return (ws[0] + ws[1]) + (ws[2] + ws[3]), (wq[0] + wq[1]) + (wq[2] + wq[3]), maxabs, float(n - int(ok.sum()))


def cut_segments(segments, n_flat=None):
    """The chunking rule of pg_segment_stats_plan in Python: ``(chunks, ranges)`` as lists of (offset, length) / (first chunk, count).
    Segment after segment in chunks of ``ops.SEG_CHUNK`` floats, the last one of a segment shorter; a chunk never spans two segments."""
    chunks, ranges = [], []
    for off, n in segments:
        off, n = int(off), int(n)
        if n < 1 or off < 0 or (n_flat is not None and off + n > n_flat):
            raise ValueError('segment (%d, %d) is empty or outside a buffer of %s floats' % (off, n, n_flat))
        if off % 4:
            raise ValueError('segment offset %d is not a multiple of 4 elements (PG_E_ALIGN)' % off)
        first = len(chunks)
        for start in range(0, n, ops.SEG_CHUNK):
            chunks.append((off + start, min(ops.SEG_CHUNK, n - start)))
        ranges.append((first, len(chunks) - first))
    return chunks, ranges


def _segments_host(flat, chunks, ranges):
    x = flat.detach().numpy().reshape(-1)
    parts = [_chunk_host(x[o:o + n]) for o, n in chunks]
    out = np.zeros((len(ranges), 4))
    for s, (first, count) in enumerate(ranges):
        for p in parts[first:first + count]:
            out[s, 0] += p[0]
            out[s, 1] += p[1]
            out[s, 2] = max(out[s, 2], p[2])
            out[s, 3] += p[3]
    return torch.from_numpy(out)


# ----------------------------------------------------------------------------------------------- objects
class ScalarStats(object):
    """Running statistics of up to ``ops.STATS_MAX_SOURCES`` named scalar series, e.g. the four losses of an iteration.

    ``push(*tensors)``: one value per name -- the mean of the tensor handed over for it (a 0-dim cost, an ``[N, 1]`` per-sample loss;
    None skips the name).  With fp32 device tensors this is ONE launch on the current stream and never synchronises: the tensors must
    have been produced on that stream (or be ordered before it), and may be freed or overwritten by later work on it.  With host
    tensors or Python floats the numpy twin folds the values at once.  An object stays with what its first push gave it.
    ``read(reset=True)``: one device-to-host copy of K x 64 bytes (it waits for the pushes before it).  Per name: ``mean``, ``std`` (the
    population standard deviation, from sum and sumsq, the variance clamped at 0), ``min``, ``max``, ``last``, ``count`` (the finite values,
    which the other five are over), ``nonfinite`` (NaN / +-Inf values: counted, and visible in ``last``, never in the sums) and
    ``first_bad`` (the 0-based index of the first of them among the name's pushes since the last reset, -1 without one).  The reset
    itself costs nothing: it travels as a flag of the next push."""

    def __init__(self, names):
        names = tuple(names)
        if not 1 <= len(names) <= ops.STATS_MAX_SOURCES or len(set(names)) != len(names):
            raise ValueError('ScalarStats: 1 .. %d distinct names, got %r' % (ops.STATS_MAX_SOURCES, names))
        self.names = names
        self._dev = None                 # float64 [K, 8] on the device | numpy [K, 8] on the host, after the first push
        self._pending_reset = True       # the next push starts from the empty record
        self.pushes = 0

    @property
    def on_device(self):
        return torch.is_tensor(self._dev)

    @property
    def empty(self):
        """Nothing was pushed since the last reset (or ever)."""
        return self._dev is None or self._pending_reset

    def push(self, *values):
        if len(values) != len(self.names):
            raise ValueError('ScalarStats.push: %d values for %d names' % (len(values), len(self.names)))
        device = all(v is None or (torch.is_tensor(v) and v.is_cuda) for v in values) and any(v is not None for v in values)
        if self._dev is None:
            first = next(v for v in values if v is not None) if device else None
            self._dev = ops.scalar_stats_record(len(self.names), first.device) if device else np.empty((len(self.names), 8))
        if device != self.on_device:
            raise TypeError('ScalarStats.push: this object was started with %s values' % ('device' if self.on_device else 'host'))
        if device:
            ops.scalar_stats_push(self._dev, values, reset=self._pending_reset)
        else:
            if self._pending_reset:
                self._dev[:] = _EMPTY
            for k, v in enumerate(values):
                if v is not None:
                    _fold_host(self._dev[k], float(_mean_host(v.detach().cpu().numpy() if torch.is_tensor(v) else v)))
        self._pending_reset = False
        self.pushes += 1

    def record(self):
        """The raw record as a float64 host array [K, 8] (``RECORD_FIELDS``); the empty record while nothing was pushed since a reset."""
        if self.empty:
            return np.array([_EMPTY] * len(self.names))
        return self._dev.cpu().numpy() if self.on_device else self._dev.copy()

    def read(self, reset=True):
        rec = self.record()
        if reset:
            self._pending_reset = True
        out = {}
        for name, r in zip(self.names, rec):
            n = r[0]
            mean = r[1] / n if n > 0 else float('nan')
            var = max(r[2] / n - mean * mean, 0.0) if n > 0 else float('nan')
            out[name] = dict(mean=float(mean), std=float(math.sqrt(var)) if n > 0 else float('nan'), min=float(r[3]), max=float(r[4]),
                             last=float(r[5]), count=int(n), nonfinite=int(r[6]), first_bad=int(r[7]))
        return out


def segments_of(net):
    """``[(name, offset, length), ...]`` of a network's flat parameter buffer: the weight and the bias of every ``PGConv2d`` and of D's
    ``linear``.  Names come from ``named_modules`` (``blocks.3.c1.weight``), offsets from ``net._flat_offsets`` (multiples of 4
    elements); the padding behind a parameter belongs to no segment."""
    from .network import PGConv2d
    if getattr(net, '_flat_param', None) is None:
        raise ValueError('segments_of: the network has no flat parameter buffer')
    off = {id(p): o for p, o in zip(net.parameters(), net._flat_offsets)}
    out = []
    for name, m in net.named_modules():
        if isinstance(m, PGConv2d):
            pairs = (('weight', m.conv.weight), ('bias', m.conv.bias))
        elif isinstance(m, torch.nn.Linear):
            pairs = (('weight', m.weight), ('bias', m.bias))
        else:
            continue
        for what, p in pairs:
            out.append(('%s.%s' % (name, what), off[id(p)], p.numel()))
    return out


class SegmentStats(object):
    """Statistics of S segments of one flat fp32 buffer.  ``segments``: ``(offset, length)`` or ``(name, offset, length)`` tuples,
    offsets multiples of 4 elements, lengths >= 1; ``n_flat``: the length of the buffers that will be measured.  The chunk table and
    the per-segment chunk ranges are made here and, for a device, uploaded here, once.
    ``measure(flat)`` -> float64 ``[S, 4]`` on ``device``: ``SEGMENT_FIELDS`` over the finite elements of every segment.  Two launches on
    the current stream, no synchronisation; bit-reproducible, and a segment's row does not depend on what the others hold."""

    segments_of = staticmethod(segments_of)

    def __init__(self, segments, device, n_flat=None):
        segments = [tuple(s) for s in segments]
        self.names = [s[0] if len(s) == 3 else str(i) for i, s in enumerate(segments)]
        self.segments = [tuple(int(v) for v in s[-2:]) for s in segments]
        if not self.segments:
            raise ValueError('SegmentStats: no segments')
        self.device = torch.device(device)
        self.n_flat = int(n_flat) if n_flat is not None else max(o + n for o, n in self.segments)
        if self.device.type == 'cpu':
            self._chunks, self._ranges = cut_segments(self.segments, self.n_flat)
            self._partials = None
        else:
            chunks, ranges = ops.segment_stats_plan(self.segments, self.n_flat)
            self._chunks, self._ranges = chunks.to(self.device), ranges.to(self.device)
            self._partials = torch.empty((chunks.shape[0], 4), device=self.device, dtype=torch.float64)
        self.nchunks = len(self._chunks)

    @classmethod
    def for_network(cls, net):
        return cls(segments_of(net), net._flat_param.device, net._flat_param.numel())

    def measure(self, flat):
        if (not torch.is_tensor(flat) or flat.dtype != torch.float32 or flat.dim() != 1 or not flat.is_contiguous()
                or flat.device.type != self.device.type or flat.numel() != self.n_flat):
            raise ValueError('SegmentStats.measure: expected a contiguous float32 vector of %d elements on %s' % (self.n_flat, self.device))
        if self.device.type == 'cpu':
            return _segments_host(flat, self._chunks, self._ranges)
        return ops.segment_stats(flat, self._chunks, self._ranges, partials=self._partials)
