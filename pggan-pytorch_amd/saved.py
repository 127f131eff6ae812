"""What a forward pass of ``engine`` hands to its backward sweeps: the saved activations of the G and D passes, the adjoints and
Hessian-vector terms the gradient-penalty sweeps pass on, and the two loss states.  Every class is closed (``__slots__``): a schedule
feature that saves something new declares it here, ONCE, in the class's ``LAYOUT`` table together with the layout of its leading extent --
``slice_rows`` / ``merge_rows`` / ``tensors`` below are driven by those tables, so a declared tensor cannot be forgotten by the
gradient-penalty slice, the three-pass merge or the cross-stream hand-over.  A field a path does not produce is None.
``Sign`` and ``PoolAdjoint`` at the end are what the D sweeps build from these records at the point of use (closed too, but never
saved, sliced or merged: no table).  Imports nothing from the package."""

import collections

import torch

# layout of a field's leading extent
IMG = 'image-major'       # rows = images: [n, ...]
PIX = 'per-pixel'         # rows = images x pixels: [n * h * w] (PixelNorm scales)
GRP = 'per-group'         # rows = minibatch-stddev groups: [groups, ...]
EACH = 'records'          # a list of records, one per block, each sliced / merged like its parent
# None                    # not batch-sliced: modules, geometry, flags, scalars


class _Record(object):
    __slots__ = ()
    LAYOUT = {}

    def __init__(self, **fields):
        for f in self.__slots__:
            setattr(self, f, None)
        for f, v in fields.items():
            setattr(self, f, v)


class GBlock(_Record):
    """One grown block of a generator pass.  Writer: engine.generator_forward; readers: generator_backward."""
    LAYOUT = {
        'blk': None,      # the GBlock module
        'H': None,        # output resolution of the block
        'inp': IMG,       # input of c1 at H/2 (the SAME tensor object as the coarser block's a2 / the context's y2); wgrad of c1, fade-in toRGB
        'a1': IMG,        # c1 output (after PixelNorm); wgrad of c2, adjoint of c1's activation
        'r1': PIX,        # c1's PixelNorm scales; None without PixelNorm
        'a2': IMG,        # c2 output (after PixelNorm); toRGB's wgrad, adjoint of c2's activation
        'r2': PIX,        # c2's PixelNorm scales; None without PixelNorm
    }
    __slots__ = tuple(LAYOUT)


class GContext(_Record):
    """A generator pass kept for its backward.  Writer: engine.generator_forward(save=True); readers: generator_backward, and
    d_step_generator / _early_g_on_side, which leave (a slice of) it in an EarlyG -- plans.g_step compares that object by identity."""
    LAYOUT = {
        'N': None,        # images
        'depth': None,    # growth stage of the pass
        'alpha': None,    # fade-in weight of the pass
        'zn': IMG,        # normalised latents (the latents themselves without normalisation); wgrad of block0.c1
        'y1': IMG,        # block0.c1 output
        'r1': PIX,        # ... its PixelNorm scales; None without PixelNorm
        'y2': IMG,        # block0.c2 output
        'r2': PIX,        # ... its PixelNorm scales
        'recs': EACH,     # GBlock per grown block, coarse to fine
    }
    __slots__ = tuple(LAYOUT)

    def slice(self, a, b):
        """Images [a, b) of the pass (views)."""
        sub = slice_rows(self, self.N, a, b)
        sub.N = b - a
        return sub


class DBlock(_Record):
    """One block of a discriminator pass.  Writer: engine.d_forward; readers: d_backward and its steps (through ``Sign.a1`` / ``a2`` /
    ``inp`` wherever only the sign of an activation is read), d_tangent_wgrad, _mbstd_bwd_hvp."""
    LAYOUT = {
        'blk': None,      # the DBlock module
        'H': None,        # input resolution of the block
        'first': None,    # the entry block of this stage (its input is fromRGB's output)
        'last': None,     # the 4x4 block (minibatch stddev, c2 is 4x4 -> 1x1)
        'inp': IMG,       # block input; None in the entry block of d_forward(keep_input=False) when fromRGB ran in c1's gather
        'inpb': IMG,      # entry block from SIGN_BYTES_MIN_H up: sign bytes of inp
        'mb': IMG,        # last block: inp with the minibatch-stddev channel
        'stats': GRP,     # last block: per-group statistics of the minibatch stddev
        'a1': IMG,        # c1 output (normalised under PixelNorm)
        'a1b': IMG,       # sign bytes of a1 where the launch produced them
        'r1': PIX,        # PixelNorm discriminator: scales of a1
        'a2': IMG,        # c2 output: fp32, or sign bytes from SIGN_BYTES_MIN_H up (only its sign is read again)
        'r2': PIX,        # PixelNorm discriminator: scales of a2
        'pf': IMG,        # entry block while fading in: the next block's fromRGB of the pooled image
    }
    __slots__ = tuple(LAYOUT)


class DContext(_Record):
    """A discriminator pass over ``groups`` stacked minibatches.  Writer: engine.d_forward, ``merge`` (three passes -> one batch),
    ``slice`` (the mixed third for the gradient penalty); readers: d_backward, d_tangent_wgrad, d_loss_backward."""
    LAYOUT = {
        'NB': None,       # images
        'groups': None,   # minibatch-stddev groups
        'depth': None,    # growth stage of the pass
        'alpha': None,    # fade-in weight of the pass
        'x': IMG,         # the NCHW image batch
        'recs': EACH,     # DBlock per block, fine to coarse
    }
    __slots__ = tuple(LAYOUT)

    def slice(self, a, b, g0, g1):
        """Images [a, b) == groups [g0, g1) of the pass (views)."""
        sub = slice_rows(self, self.NB, a, b, g0, g1)
        sub.NB, sub.groups = b - a, g1 - g0
        return sub

    @classmethod
    def merge(cls, parts):
        """The context of the whole batch from those of its passes: every tensor of a pass is a row range of ONE batched tensor."""
        ctx = merge_rows(parts)
        ctx.NB, ctx.groups = sum(p.NB for p in parts), sum(p.groups for p in parts)
        return ctx


class DAdjoint(_Record):
    """First-backward adjoints of one block under the gradient penalty.  Writer: d_backward(save_adjoints=True) (gy1 / gy2: _pn_adjoints);
    reader: d_tangent_wgrad (the other factor of every tangent weight gradient)."""
    LAYOUT = {
        'gz2': IMG,       # adjoint of c2's pre-activation
        'gz1': IMG,       # adjoint of c1's pre-activation
        'gmb': IMG,       # last block: adjoint of the minibatch-stddev output (Hvp.gy_first)
        'gf': IMG,        # entry block: adjoint of fromRGB's pre-activation
        'gpf': IMG,       # entry block while fading in: adjoint of the next block's fromRGB pre-activation
        'gy1': IMG,       # PixelNorm discriminator: adjoint of the normalised a1 (copy)
        'gy2': IMG,       # PixelNorm discriminator: adjoint of the normalised a2 (copy)
    }
    __slots__ = tuple(LAYOUT)


class PNInjection(_Record):
    """PixelNorm Hessian-vector injections of one block.  Writer: d_tangent_wgrad (ops.pixelnorm_tangent); reader: _pn_adjoints."""
    LAYOUT = {
        'inj1': IMG,      # added to the adjoint of a1's (LeakyReLU -> PixelNorm) on the mixed images
        'inj2': IMG,      # ... of a2's
    }
    __slots__ = tuple(LAYOUT)


class Hvp(_Record):
    """Hessian-vector bundle of the gradient penalty: the last ``NB - n_head`` images of the batched sweep form one extra group whose
    score gradient is zero and which receives these injections.  Writer: d_tangent_wgrad (d_loss_backward adds n_head); readers:
    d_backward, _mbstd_bwd_hvp."""
    LAYOUT = {
        'n_head': None,   # images in front of the mixed ones ([real | fake]: 2N)
        'tx': IMG,        # tangent of the minibatch-stddev input
        'tstats': GRP,    # tangent statistics (ops.mbstd_tangent)
        'gy_first': IMG,  # first-backward adjoint of the minibatch-stddev output (DAdjoint.gmb)
        'injs': EACH,     # PNInjection per block; None without a PixelNorm discriminator
    }
    __slots__ = tuple(LAYOUT)


class DLossState(_Record):
    """Writer: engine.d_loss_forward; reader: d_loss_backward (and diagnostics: tools/, tests/test_fp64_adjudicator.py).
    For an objective without a penalty (engine._d_plain_loss_forward) D, N, ctx over [real | fake], gscore and scores only: the reader then
    skips the tangent pass."""
    LAYOUT = {
        'D': None,          # the discriminator
        'N': None,          # minibatch size
        'ctx': None,        # DContext of the [real | fake | mixed] batch
        'sub': None,        # ... its mixed third (views), the gradient penalty's pass
        'adj': None,        # [DAdjoint] of the gradient penalty's first backward over ``sub``
        'u': IMG,           # seed of the tangent pass (ops.gp_seed), shaped like the mixed images
        'gscore': IMG,      # d loss / d score
        'scores': IMG,      # D's scores of the 3N images
        'gp': IMG,          # gradient penalty per mixed image
        'arena_use': None,  # _ArenaUse token while ctx aliases the network's three-pass buffers; None: freshly allocated
        'arena_st': None,   # ... those _DForwardBuffers
    }
    __slots__ = tuple(LAYOUT)


class GLossState(_Record):
    """Writer: engine.g_loss_forward; reader: g_loss_backward, which leaves ``active_g`` for plans.g_step / graphs.g_step."""
    LAYOUT = {
        'G': None,          # the generator
        'D': None,          # the discriminator
        'gctx': None,       # GContext of G(z)
        'dctx': None,       # DContext of D(G(z)), keep_input=False
        'gscore': IMG,      # d loss / d score
        'table': IMG,       # int32 [N, 8] augmentation table the forward applied to G(z) (None: no Augmenter); the backward transposes with it
        'active_g': None,   # layers of G that received a gradient (generator_backward)
    }
    __slots__ = tuple(LAYOUT)


def _copy(rec):
    out = object.__new__(type(rec))
    for f in rec.__slots__:
        setattr(out, f, getattr(rec, f))
    return out


def slice_rows(rec, n, a, b, g0=None, g1=None):
    """Copy of ``rec`` (a record over ``n`` images) whose declared tensors are the views of images [a, b) == groups [g0, g1)."""
    out = _copy(rec)
    for f, layout in rec.LAYOUT.items():
        v = getattr(rec, f)
        if v is None or layout is None:
            continue
        if layout is EACH:
            v = [slice_rows(r, n, a, b, g0, g1) for r in v]
        elif layout is GRP:
            v = v[g0:g1]
        else:                                        # IMG: one row per image; PIX: h * w rows per image
            per = v.shape[0] // n
            v = v[a * per:b * per]
        setattr(out, f, v)
    return out


def _whole(a, *bs):
    base = a._base if a._base is not None else a
    if all(b is not None and b._base is base for b in bs) and base.shape[0] == a.shape[0] + sum(b.shape[0] for b in bs):
        return base
    raise RuntimeError('split D forward: the passes did not write into one tensor')


def merge_rows(parts):
    """Inverse of ``slice_rows`` over consecutive row ranges: the record whose declared tensors are the base tensors the parts view."""
    first = parts[0]
    out = _copy(first)
    for f, layout in first.LAYOUT.items():
        v = getattr(first, f)
        if v is None or layout is None:
            continue
        if layout is EACH:
            v = [merge_rows([getattr(p, f)[i] for p in parts]) for i in range(len(v))]
        else:
            v = _whole(*[getattr(p, f) for p in parts])
        setattr(out, f, v)
    return out


def tensors(rec, seen=None):
    """Every declared tensor of ``rec`` and its block records, each distinct tensor object once (a block's ``inp`` IS the coarser
    block's ``a2``)."""
    seen = set() if seen is None else seen
    for f, layout in rec.LAYOUT.items():
        v = getattr(rec, f)
        if v is None or layout is None:
            continue
        if layout is EACH:
            for r in v:
                for t in tensors(r, seen):
                    yield t
        elif id(v) not in seen:
            seen.add(id(v))
            yield v


class Sign(collections.namedtuple('Sign', 'f32 bytes slope', defaults=(None, None, 0.2))):
    """The sign of an activation, i.e. its LeakyReLU' mask: the fp32 activation, its sign bytes (1 byte per 4 channels), or both.  Built
    from a DBlock where a mask is needed (an immutable triple: one is made per mask per sweep, on the eager path's host time);
    engine._bytes_first is the one place that chooses between the two forms."""
    __slots__ = ()

    @classmethod
    def a1(cls, rec, n=None):
        """c1's output (its first ``n`` images: the 4x4 block under the gradient penalty)."""
        if n is None:
            return cls(rec.a1, rec.a1b, rec.blk.c1.slope)
        return cls(rec.a1[:n], None if rec.a1b is None else rec.a1b[:n], rec.blk.c1.slope)

    @classmethod
    def a2(cls, rec):
        """c2's output, kept in ONE of the two forms (DBlock.a2)."""
        b = rec.a2.dtype == torch.uint8
        return cls(None if b else rec.a2, rec.a2 if b else None, rec.blk.c2.slope)

    @classmethod
    def inp(cls, rec):
        """The entry block's input (fromRGB's output)."""
        return cls(rec.inp, rec.inpb, rec.blk.fromRGB.slope)


class PoolAdjoint(object):
    """What a block of the D adjoint sweep hands to the next finer block's c2.  Producer: engine._hand_over (and d_backward's head);
    consumers: engine._consume / _pn_adjoints.  Either evaluated -- ``g``, the adjoint of c2's pre-activation (of its normalised output
    under PixelNorm) -- or lazy: the gradient ``coarse`` of the pooled map, for c2's consumers to unpool in their gathers as
    4 * ``mul`` * LeakyReLU'(``up``) * nearest-upsample(coarse), ``up`` being the Sign (bytes) of the finer c2's output."""
    __slots__ = ('g', 'coarse', 'up', 'mul')

    def __init__(self, g=None, coarse=None, up=None, mul=None):
        if not ((coarse is None and up is None and mul is None) if g is not None else
                (coarse is not None and mul is not None and up is not None and up.bytes is not None)):
            raise ValueError('a pool adjoint is either evaluated (g) or lazy (coarse, up with sign bytes, mul)')
        self.g, self.coarse, self.up, self.mul = g, coarse, up, mul
