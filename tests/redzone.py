"""TEST INFRASTRUCTURE: guard bands around the tensors handed to a kernel (docs/experiments_redzone.md).

Every tensor of the per-kernel tiers is its own allocation: 512-byte aligned, with whatever the caching allocator put next
to it.  A store past the end of an output, a load from outside an input, an output element that is never written, a write
to an input and a reliance on more than the 16-byte alignment of the contract (include/pggan_hip.h, "16-byte aligned
bases") are all invisible there.  ``Redzone.guard`` copies a tensor into the middle of one larger allocation

    [ lead band: 1 MiB + 16 bytes | payload | tail band: 1 MiB ]

so that the payload is 16-byte aligned AND NO BETTER and the tail band starts at the payload's last byte (a ``[3]`` bias
gets no slack).  1 MiB is a condition, not a measurement: several times the largest tile row a ragged-tail overrun can
span (64 pixels x 512 channels x 4 bytes = 128 KiB).  Band contents by kind:

    'data'   fp32 / fp64 operands: NaN -- an outside load that reaches the result poisons it, the parity assertion fails
    'mask'   operands consumed through a comparison (fp32 masks, sign bytes): NaN would be swallowed by ``mask > 0``, so
             the caller runs twice, with bands that read as positive (+1.0 / 0xFF) and as negative (-1.0 / 0x00)
    'acc'    operands a kernel ADDS into (dw / db / gimg, atomics): a finite 1.29.. with a distinctive mantissa -- an add that
             lands in a NaN band would leave its bits as they were
    outputs  the whole allocation, payload included, holds a sentinel no kernel produces (a NaN with a distinctive
             payload; 0xA5 for sign bytes, which only use the low nibble)

``Redzone.check`` then compares bitwise on the device: every band unchanged, every input payload unchanged (the in-place
operands are named by the caller), no element of an output still the sentinel.  ``AllocatorProxy`` stands in for the
``torch`` name of a module (``monkeypatch.setattr(pg.ops, 'torch', rz.proxy())``) so that the outputs the wrappers create
themselves are guarded too; it changes no product code.  Device-agnostic: tests/test_redzone_host.py runs it on the CPU."""
import sys

import torch

LEAD = (1 << 20) + 16
TAIL = 1 << 20

_NAN32 = (0x00, 0x00, 0xC0, 0x7F)                               # 0x7FC00000
_NAN64 = (0, 0, 0, 0, 0, 0, 0xF8, 0x7F)
_SENT32 = (0xA5, 0xA5, 0xC5, 0x7F)                              # 0x7FC5A5A5: a quiet NaN no arithmetic produces
_SENT64 = (0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xF8, 0x7F)
_ACC32 = (0xA5, 0xA5, 0xA5, 0x3F)                               # 0x3FA5A5A5 = 1.2941...: any add of more than 6e-8 changes it
_ACC64 = (0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xF4, 0x3F)
_ONE32 = {1: (0x00, 0x00, 0x80, 0x3F), -1: (0x00, 0x00, 0x80, 0xBF)}
SENTINEL_U8 = (0xA5, 0x5A)                                      # uint8 image outputs, where 0xA5 is a legal value: run with both

POLARITIES = (1, -1)


class RedzoneError(AssertionError):
    """A kernel touched a band, modified an input or left an output element unwritten."""


def _pattern(dtype, kind, polarity):
    if kind == 'out':
        if dtype in (torch.float32, torch.float64):
            return _SENT32 if dtype == torch.float32 else _SENT64
        return (SENTINEL_U8[0 if polarity >= 0 else 1],) * torch.empty((), dtype=dtype).element_size()      # one pattern per ELEMENT
    if kind == 'mask':
        if dtype == torch.float32:
            return _ONE32[polarity]
        return (0xFF,) if polarity > 0 else (0x00,)
    if kind == 'acc':
        return {torch.float32: _ACC32, torch.float64: _ACC64}[dtype]
    if kind != 'data':
        raise ValueError('kind must be data / mask / acc, got %r' % (kind,))
    return {torch.float32: _NAN32, torch.float64: _NAN64}.get(dtype, (0x7F,) * torch.empty((), dtype=dtype).element_size())   # integers: large positive


class _Record(object):
    def __init__(self, name, role, raw, off, nbytes, view, pattern, expected, must_write):
        self.name, self.role, self.raw, self.off, self.nbytes, self.view = name, role, raw, off, nbytes, view
        self.pattern, self.expected, self.must_write = pattern, expected, must_write


class Redzone(object):
    def __init__(self, device):
        self.device = torch.device(device)
        self.records = []
        self._n = 0
        self.site_counts = {}                                   # AllocatorProxy: outputs created per calling function since the last check

    # ------------------------------------------------------------------------------------------- allocation
    def _alloc(self, shape, dtype, pattern):
        nbytes = int(torch.Size(shape).numel()) * torch.empty((), dtype=dtype).element_size()
        P = len(pattern)
        total = LEAD + nbytes + TAIL + 64
        total += -total % P
        raw = torch.empty(total, dtype=torch.uint8, device=self.device)
        off = LEAD + (16 - (raw.data_ptr() + LEAD)) % 32       # payload pointer = 16 (mod 32)
        assert off % P == 0 and off + nbytes + TAIL <= total
        raw.copy_(torch.tensor(pattern, dtype=torch.uint8, device=self.device).repeat(total // P))
        view = raw[off:off + nbytes].view(dtype).view(torch.Size(shape))
        assert view.data_ptr() % 16 == 0 and view.data_ptr() % 32 != 0 and view.is_contiguous()
        return raw, off, nbytes, view

    def _name(self, name, what):
        self._n += 1
        return name if name is not None else '%s#%d' % (what, self._n)

    def guard(self, t, kind='data', polarity=1, name=None, inplace=False):
        """Copy ``t`` (any device) between two bands; returns the contiguous, 16-byte-and-no-better aligned view.
        ``inplace``: a documented in-place operand (adam's p / m / v, ema's avg, accumulating dw / db / gimg, inplace=True):
        its bands are checked, its payload is not."""
        if t is None:
            return None
        if kind == 'acc':
            inplace = True
        pattern = _pattern(t.dtype, kind, polarity)
        raw, off, nbytes, view = self._alloc(t.shape, t.dtype, pattern)
        view.copy_(t)
        self.records.append(_Record(self._name(name, 'input'), 'inout' if inplace else 'in', raw, off, nbytes, view, pattern,
                                    raw.clone(), False))
        return view

    def out(self, shape, dtype=torch.float32, name=None, fill=None, sentinel=0):
        """An output between two bands.  ``fill`` None: sentinel everywhere (``sentinel`` 1: the second uint8 pattern) and
        ``check`` demands that every element was written; a number: the payload holds it (``zeros`` / accumulating outputs)."""
        pattern = _pattern(dtype, 'out', 1 if sentinel == 0 else -1)
        raw, off, nbytes, view = self._alloc(shape, dtype, pattern)
        if fill is not None:
            view.fill_(fill)
        self.records.append(_Record(self._name(name, 'output'), 'out', raw, off, nbytes, view, pattern, raw.clone(), fill is None))
        return view

    def proxy(self, real=torch, helpers=()):
        return AllocatorProxy(self, real, helpers)

    # ------------------------------------------------------------------------------------------------ check
    @staticmethod
    def _span(diff):
        idx = diff.nonzero()
        return int(idx[0]), int(idx[-1]), int(idx.numel())

    def check(self, may_stay_unwritten=(), keep_outputs=False):
        """Synchronise, then: bands of every record unchanged; payload of every plain input unchanged; no element of an output
        still the sentinel (outputs named in ``may_stay_unwritten`` -- by record name or by tensor -- excepted).  Output
        records are dropped afterwards (``keep_outputs`` keeps them for a later check), inputs stay."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        errors = []
        exempt_names = set(e for e in may_stay_unwritten if isinstance(e, str))
        exempt_ptrs = set(e.data_ptr() for e in may_stay_unwritten if torch.is_tensor(e))
        for r in self.records:
            end = r.off + r.nbytes
            if not torch.equal(r.raw[:r.off], r.expected[:r.off]):
                first, last, n = self._span(r.raw[:r.off] != r.expected[:r.off])
                errors.append('%s: lead band touched, %d bytes, from %d to %d bytes BEFORE the payload' % (r.name, n, r.off - first, r.off - last))
            if not torch.equal(r.raw[end:], r.expected[end:]):
                first, last, n = self._span(r.raw[end:] != r.expected[end:])
                errors.append('%s: tail band touched, %d bytes, from byte %d to byte %d PAST the payload end' % (r.name, n, first, last))
            if r.role == 'in' and not torch.equal(r.raw[r.off:end], r.expected[r.off:end]):
                first, last, n = self._span(r.raw[r.off:end] != r.expected[r.off:end])
                errors.append('%s: input payload modified, %d bytes, first at byte %d, last at byte %d' % (r.name, n, first, last))
            if r.role == 'out' and r.must_write and r.name not in exempt_names and r.view.data_ptr() not in exempt_ptrs and r.nbytes:
                P = len(r.pattern)
                sent = torch.tensor(r.pattern, dtype=torch.uint8, device=self.device)
                left = (r.raw[r.off:end].view(-1, P) == sent).all(dim=1)
                if bool(left.any()):
                    first, last, n = self._span(left)
                    errors.append('%s %s: %d of %d elements never written, first element %d, last element %d'
                                  % (r.name, tuple(r.view.shape), n, left.numel(), first, last))
        self.site_counts = {}
        if not keep_outputs:
            self.records = [r for r in self.records if r.role != 'out']
        if errors:
            raise RedzoneError('; '.join(errors))

    def discard_outputs(self):
        """Drop the output records of a call that was refused before it launched (ops.Unsupported)."""
        self.records = [r for r in self.records if r.role != 'out']
        self.site_counts = {}

    def forget(self):
        self.records = []
        self.site_counts = {}


class AllocatorProxy(object):
    """Stands in for the ``torch`` name of a module: ``empty``, ``empty_like`` and ``zeros`` return recorded guarded views, every
    other attribute is the real module's.  A record is named '<calling function>:<ordinal since the last check>'; the calling
    function is the first frame outside this file that is not one of ``helpers`` (function objects of the patched module that
    allocate on behalf of their caller, e.g. ``ops._empty``, ``ops.Arena.take``: passed as objects, so a rename is an error, not
    a silent change of names).  Only what the patched module is known to ask for is served: ``dtype`` and a ``device`` of the
    Redzone's type.  An allocation for another device is forwarded to the real module unchanged; any other keyword
    (``out=``, ``pin_memory=``, ``memory_format=`` ...) is a TypeError, because serving it differently would change the module."""

    def __init__(self, rz, real=torch, helpers=()):
        self.__dict__['_rz'] = rz
        self.__dict__['_real'] = real
        self.__dict__['_helpers'] = tuple(getattr(h, '__func__', h).__code__ for h in helpers)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _new(self, shape, dtype, fill):
        f = sys._getframe(1)
        while f is not None and (f.f_code.co_filename == __file__ or f.f_code in self._helpers):
            f = f.f_back
        fn = f.f_code.co_name if f is not None else '?'
        n = self._rz.site_counts.get(fn, 0)
        self._rz.site_counts[fn] = n + 1
        return self._rz.out(shape, dtype, name='%s:%d' % (fn, n), fill=fill)

    def _elsewhere(self, what, kw, like=None):
        """True: the request is for another device (forward it).  Raises on a keyword this proxy does not serve."""
        extra = set(kw) - {'device', 'dtype'}
        if extra:
            raise TypeError('redzone allocator proxy: %s(%s=...) is not served' % (what, sorted(extra)[0]))
        dev = kw.get('device', like.device if like is not None else None)
        if dev is None:
            dev = 'cpu'                                          # torch's default device
        return torch.device(dev).type != self._rz.device.type

    def empty(self, *args, **kw):
        if self._elsewhere('empty', kw):
            return self._real.empty(*args, **kw)
        p = self._real.empty(*args, dtype=kw.get('dtype'), device='meta')
        return self._new(p.shape, p.dtype, None)

    def zeros(self, *args, **kw):
        if self._elsewhere('zeros', kw):
            return self._real.zeros(*args, **kw)
        p = self._real.empty(*args, dtype=kw.get('dtype'), device='meta')
        return self._new(p.shape, p.dtype, 0)

    def empty_like(self, t, **kw):
        if self._elsewhere('empty_like', kw, like=t):
            return self._real.empty_like(t, **kw)
        if not t.is_contiguous():
            raise TypeError('redzone allocator proxy: empty_like of a non-contiguous tensor is not served')
        return self._new(t.shape, kw.get('dtype', t.dtype), None)
