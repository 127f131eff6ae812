"""The guard-band harness (tests/redzone.py) proves itself on the CPU: fake "ops" written here as plain torch on CPU tensors.
Every negative case must FAIL the harness (pytest.raises on its own error) -- the evidence that a green run of a guarded
GPU test means something."""
import types

import pytest
import torch

import redzone
from redzone import Redzone, RedzoneError


def flat_bytes(view, rz):
    """The uint8 allocation behind a guarded view and the payload's offset in it (what an out-of-bounds kernel would index)."""
    for r in rz.records:
        if r.view.data_ptr() == view.data_ptr():
            return r.raw, r.off, r.nbytes
    raise KeyError('not a guarded view of this Redzone')


def flat_f32(view, rz, start, count):
    """``count`` floats starting ``start`` elements from the payload's first one (negative: in the lead band)."""
    raw, off, _ = flat_bytes(view, rz)
    return raw[off + 4 * start:off + 4 * (start + count)].view(torch.float32)


def scale_op(x, y):
    y.copy_(x * 2)


def test_well_behaved_op_passes():
    rz = Redzone('cpu')
    x = rz.guard(torch.randn(5, 7))
    y = rz.out((5, 7))
    scale_op(x, y)
    rz.check()
    assert torch.equal(y, x * 2)
    assert [r.role for r in rz.records] == ['in']            # outputs are dropped after a check, inputs stay ...
    rz.check()                                                # ... and stay checked


def test_payload_is_16_byte_aligned_and_no_better():
    rz = Redzone('cpu')
    for shape, dt in (((3,), torch.float32), ((2, 3, 5, 5), torch.float32), ((7,), torch.uint8), ((4, 4), torch.float64), ((9, 2), torch.int32)):
        for v in (rz.guard(torch.zeros(shape, dtype=dt)), rz.out(shape, dt)):
            assert v.data_ptr() % 16 == 0 and v.data_ptr() % 32 != 0
            assert v.is_contiguous() and tuple(v.shape) == shape and v.dtype == dt
            raw, off, nbytes = flat_bytes(v, rz)
            assert off >= (1 << 20) + 16 and raw.numel() - off - nbytes >= (1 << 20)


def test_one_float_past_the_payload_is_caught_with_its_offset():
    rz = Redzone('cpu')
    x = rz.guard(torch.randn(8))
    y = rz.out((8,))
    scale_op(x, y)
    flat_f32(y, rz, 8 + 5, 1).fill_(1.0)                      # element 13 of an 8-element output
    with pytest.raises(RedzoneError, match=r'tail band touched, 4 bytes, from byte 20 to byte 23 PAST'):
        rz.check()


def test_one_byte_before_the_payload_is_caught():
    rz = Redzone('cpu')
    y = rz.out((8,))
    y.fill_(0.5)
    raw, off, _ = flat_bytes(y, rz)
    raw[off - 1] = 0
    with pytest.raises(RedzoneError, match=r'lead band touched, 1 bytes, from 1 to 1 bytes BEFORE'):
        rz.check()


def test_three_element_payload_has_no_slack():
    rz = Redzone('cpu')
    b = rz.guard(torch.randn(3), 'acc')                       # a [3] bias gradient: 12 bytes, not a multiple of 16
    flat_f32(b, rz, 0, 4).add_(0.5)                           # a float4 add over elements 0..3 ('acc' bands are finite: an add shows)
    with pytest.raises(RedzoneError, match=r'tail band touched, 1 bytes, from byte 2 to byte 2 PAST'):   # 0x3FA5A5A5 + 0.5 = 0x3FE5A5A5
        rz.check()
    rz = Redzone('cpu')
    s = rz.out((5,), torch.uint8)                             # sign bytes
    raw, off, nbytes = flat_bytes(s, rz)
    raw[off:off + 8] = 3                                      # an 8-byte store over 5 bytes
    with pytest.raises(RedzoneError, match=r'tail band touched, 3 bytes, from byte 0 to byte 2 PAST'):
        rz.check()


def test_unwritten_output_element_is_caught():
    for dt in (torch.float32, torch.float64, torch.uint8):
        rz = Redzone('cpu')
        y = rz.out((4, 6), dt, name='y')
        y.fill_(1)
        flat = y.view(-1)
        raw, off, nbytes = flat_bytes(y, rz)
        es = flat.element_size()
        raw[off + 17 * es:off + 18 * es] = rz.records[-1].expected[off + 17 * es:off + 18 * es]      # element 17 keeps the sentinel
        with pytest.raises(RedzoneError, match=r'y \(4, 6\): 1 of 24 elements never written, first element 17, last element 17'):
            rz.check(keep_outputs=True)
        rz.check(may_stay_unwritten=('y',), keep_outputs=True)                # exempt by name ...
        rz.check(may_stay_unwritten=(y,))                                     # ... or by tensor
    rz = Redzone('cpu')
    c = rz.out((6,), torch.int32, name='c')                                   # wider integers: one sentinel per ELEMENT, not per byte
    c.copy_(torch.tensor([0xA5, 0x5AA5, -1, 0, 0xA5A5A5, 7], dtype=torch.int32))     # written values that contain 0xA5 bytes
    rz.check(keep_outputs=True)
    raw, off, _ = flat_bytes(c, rz)
    raw[off + 16:off + 20] = 0xA5
    with pytest.raises(RedzoneError, match=r'c \(6,\): 1 of 6 elements never written, first element 4, last element 4'):
        rz.check()
    rz = Redzone('cpu')
    rz.out((4,), fill=0.0)                                                    # pre-filled (accumulating / zeros): nothing to demand
    rz.check()
    rz = Redzone('cpu')
    g = rz.out((4,), torch.uint8, sentinel=1)                                 # uint8 images: 0xA5 is a legal value, so a second sentinel
    g.fill_(0xA5)
    rz.check()


def test_fp32_sentinel_is_a_nan_no_kernel_writes():
    rz = Redzone('cpu')
    y = rz.out((4,))
    assert bool(torch.isnan(y).all())
    y.copy_(torch.tensor([float('nan'), 0.0, float('inf'), 1.0]))            # an ordinary NaN counts as written
    rz.check()
    y64 = rz.out((3,), torch.float64)
    assert bool(torch.isnan(y64).all())


def test_modified_input_is_caught_and_inplace_operands_are_excepted():
    rz = Redzone('cpu')
    x = rz.guard(torch.randn(6), name='x')
    x[4] += 1.0
    with pytest.raises(RedzoneError, match=r'x: input payload modified, .* first at byte 1[6-9]'):
        rz.check()
    rz = Redzone('cpu')
    p = rz.guard(torch.randn(6), inplace=True)
    p.mul_(0.5)
    rz.check()
    flat_f32(p, rz, -1, 1).fill_(0.0)                         # in-place operands still have bands
    with pytest.raises(RedzoneError, match='lead band touched'):
        rz.check()


def test_data_read_from_a_band_poisons_the_result():
    rz = Redzone('cpu')
    x = rz.guard(torch.randn(8))
    for start in (-1, 1):                                     # a window that begins one element early / ends one element late
        y = rz.out((8,))
        y.copy_(flat_f32(x, rz, start, 8) * 2)
        rz.check()                                            # nothing was written out of place ...
        assert bool(torch.isnan(y).any())                     # ... the parity assertion is what fails
    x64 = rz.guard(torch.randn(8, dtype=torch.float64))
    raw, off, _ = flat_bytes(x64, rz)
    assert bool(torch.isnan(raw[off - 8:off].view(torch.float64)).all())


def test_mask_read_from_a_band_fails_exactly_one_polarity():
    g, m = torch.randn(8), torch.tensor([1., 1., 1., 1., 1., 1., 1., 1.])     # every true mask element is positive
    want = g.clone()

    def bad_masked(gv, mv, rz, y):
        mm = flat_f32(mv, rz, 1, 8)                           # reads mask[1..8]: element 8 is the tail band
        y.copy_(gv * torch.where(mm > 0, torch.ones(8), torch.full((8,), 0.2)))

    failed = []
    for pol in redzone.POLARITIES:
        rz = Redzone('cpu')
        gv, mv = rz.guard(g), rz.guard(m, 'mask', pol)
        y = rz.out((8,))
        bad_masked(gv, mv, rz, y)
        rz.check()
        failed.append(not torch.equal(y, want))
    assert failed == [False, True]                            # the band that reads as positive hides it, the negative one shows it
    # sign bytes: 0xFF / 0x00
    for pol, byte in ((1, 0xFF), (-1, 0x00)):
        rz = Redzone('cpu')
        b = rz.guard(torch.full((5,), 0x0F, dtype=torch.uint8), 'mask', pol)
        raw, off, n = flat_bytes(b, rz)
        assert int(raw[off + n]) == byte and int(raw[off - 1]) == byte
    with pytest.raises(ValueError):
        Redzone('cpu').guard(g, 'nonsense')


def test_allocator_proxy_on_a_stand_in_module():
    mod = types.ModuleType('fake_ops')
    mod.torch = torch

    def op(x):
        y = mod.torch.empty(x.shape, device=x.device, dtype=mod.torch.float32)
        z = mod.torch.empty_like(x)
        acc = mod.torch.zeros((2, 3), device=x.device)
        b = mod.torch.empty(5, dtype=mod.torch.uint8)
        s = mod.torch.empty((), dtype=mod.torch.float64)
        y.copy_(x)
        z.copy_(mod.torch.where(x > 0, x, x * 0.2))
        b.fill_(1)
        s.fill_(2.0)
        return y, z, acc, b, s
    mod.op = op
    rz = Redzone('cpu')
    real = mod.torch
    mod.torch = rz.proxy()
    try:
        assert mod.torch.float32 is torch.float32 and mod.torch.where is torch.where and mod.torch.is_tensor(torch.ones(1))   # forwarded
        x = rz.guard(torch.randn(4, 4))
        outs = mod.op(x)
        recs = [r for r in rz.records if r.role == 'out']
        assert [r.name for r in recs] == ['op:0', 'op:1', 'op:2', 'op:3', 'op:4']
        for o, r in zip(outs, recs):
            assert o.data_ptr() == r.view.data_ptr() and o.data_ptr() % 16 == 0 and o.data_ptr() % 32 != 0
        assert [tuple(o.shape) for o in outs] == [(4, 4), (4, 4), (2, 3), (5,), ()]
        assert [o.dtype for o in outs] == [torch.float32, torch.float32, torch.float32, torch.uint8, torch.float64]
        assert bool((outs[2] == 0).all())
        rz.check()
        assert not [r for r in rz.records if r.role == 'out']

        def lazy(x):                                          # an op that forgets its second output
            y = mod.torch.empty_like(x)
            z = mod.torch.empty_like(x)
            y.copy_(x)
            return y, z
        lazy(x)
        with pytest.raises(RedzoneError, match=r'lazy:1 \(4, 4\): 16 of 16 elements never written'):
            rz.check(keep_outputs=True)
        rz.check(may_stay_unwritten=('lazy:1',))

        # a helper that allocates on behalf of its caller (ops._empty, Arena.take) is skipped when given as an OBJECT
        def _alloc(shape):
            return mod.torch.empty(shape)

        def through_helper():
            return _alloc((3,)).fill_(1.0)
        through_helper()
        assert rz.records[-1].name == '_alloc:0'
        rz.check()
        mod.torch = rz.proxy(helpers=(_alloc,))
        through_helper()
        assert rz.records[-1].name == 'through_helper:0'
        rz.check()
        # a request for another device is forwarded untouched; a keyword the proxy does not serve is an error, not a silent change
        meta = mod.torch.empty((2, 2), device='meta')
        assert meta.device.type == 'meta' and not [r for r in rz.records if r.role == 'out']
        assert mod.torch.zeros(3, device='meta').device.type == 'meta'
        assert mod.torch.empty_like(torch.empty(2, device='meta')).device.type == 'meta'
        for bad in (lambda: mod.torch.empty(3, pin_memory=True), lambda: mod.torch.zeros(3, out=torch.empty(3)),
                    lambda: mod.torch.empty_like(x, memory_format=torch.preserve_format)):
            with pytest.raises(TypeError, match='is not served'):
                bad()
        with pytest.raises(TypeError, match='non-contiguous'):
            mod.torch.empty_like(torch.zeros(4, 4).t())
    finally:
        mod.torch = real
