"""Device-resident real-image datasets: the reference's ``DepthDataset`` protocol (dataset.py:31-70) on uint8 images that live in
HBM, with the whole batch -- gather, pyramid level, mirror, fade-in, dynamic range -- in one launch of csrc/real_batch.hip.  Nothing
crosses PCIe per step and no host worker prepares anything, so the stale ``dataset.alpha`` of forked DataLoader workers
cannot occur: every batch is made with the depth and alpha of the moment it is drawn.

``DeviceImageDataset`` holds a stack [M,C,R,R] and draws image indices (``IndexStream``, ``ops.real_batch_u8``).
``DeviceStripDataset`` holds recordings of arbitrary length, each one uint8 spectrogram strip (``StripLevel``), and draws windows at
random time offsets, cut where the strip lies (``CropStream``, ``ops.crop_batch_u8``).  Both are a ``_DeviceDataset``, which owns the
stage, the training stream and the batch protocol, and both streams are an ``_EpochStream``, which owns the cursor rules; the two
batch kernels are one pair, instantiated for the two sources.

``device='cpu'`` (host mode) evaluates the same definition with numpy in fp64, as the reference computes it; it backs
``__getitem__`` and is the twin the device path is compared with, bit for bit (tests/golden/io_steps.npz pins both)."""
import os

import numpy as np
import torch

UPLOAD_CHUNK_BYTES = 256 << 20          # the stack is uploaded in pieces of at most this size: no host copy of the whole set is made


# ------------------------------------------------------------------------------------------------ host definition
def level_host(images_u8, depthdiff, range_in=(0, 255)):
    """Pyramid level ``depthdiff`` below a uint8 array [..., S, S] (create_datapoint_from_depth, dataset.py:243-250): the four
    samples at (y st + {0,1}, x st + {0,1}), st = 2^depthdiff, added in fp32 in the reference's order, / 4, rounded half to even,
    clipped to ``range_in``, uint8.  ``depthdiff == 0`` is the array itself."""
    x = np.asarray(images_u8)
    if depthdiff == 0:
        return x
    d = x.astype(np.float32)
    st = 2 ** int(depthdiff)
    acc = 0
    for a in range(2):
        for b in range(2):
            acc = acc + d[..., a::st, b::st]
    acc = acc / 4
    return np.uint8(np.clip(np.round(acc), np.float32(range_in[0]), np.float32(range_in[1])))


def prepare_host(level_u8, alpha, range_in=(0, 255), range_out=(-1, 1)):
    """DepthDataset.__getitem__ (dataset.py:54-67) for a uint8 array [..., r, r]: fade with the 2x2 box-filtered copy when
    ``alpha < 1`` (:109-113), adjust_dynamic_range (utils.py:24-30), float32 -- everything in fp64, rounded once."""
    d = np.asarray(level_u8).astype(np.float64)
    if alpha < 1.0:
        lead, r = d.shape[:-2], d.shape[-1]
        t = d.reshape(lead + (r // 2, 2, r // 2, 2)).mean((-3, -1)).repeat(2, -2).repeat(2, -1)
        d = d + (t - d) * (1.0 - float(alpha))
    lo_in, hi_in, lo_out, hi_out = (float(v) for v in tuple(range_in) + tuple(range_out))
    if (lo_in, hi_in) != (lo_out, hi_out):
        scale = (hi_out - lo_out) / (hi_in - lo_in)
        d = (d - lo_in) * scale + lo_out
    return d.astype(np.float32)


def batch_host(stack_u8, idx, flip, depthdiff, alpha, range_in=(0, 255), range_out=(-1, 1)):
    """What ``ops.real_batch_u8`` computes, on the host: a float32 array [n,C,r,r]."""
    level = level_host(np.asarray(stack_u8)[np.asarray(idx)], depthdiff, range_in)
    if flip is not None:
        f = np.asarray(flip).astype(bool)
        level = np.where(f[:, None, None, None], level[..., ::-1], level)       # the mirror acts on the LEVEL image
    return prepare_host(level, alpha, range_in, range_out)


# -------------------------------------------------------------------------------------------------------- streams
class _EpochStream(object):
    """The positions 0, 1, 2, ... of an endless sequence made of epochs of ``size`` positions.  A subclass gives ``_host_epoch()``:
    the host tensors [size] of the NEXT epoch as a tuple (``None`` for a member it does not carry); epochs are made in order.  An
    epoch's arrays are made once and moved to ``device`` once; ``take`` hands out slices of them (concatenated on the device across
    an epoch boundary): no copy and no synchronisation per batch.  ``cursor`` is the next unread position."""

    def __init__(self, size, what, shuffle, flags, device):
        self._size, self._what = int(size), what
        self.shuffle, self.flags, self.device = bool(shuffle), bool(flags), torch.device(device)
        self._epochs = {}                # epoch number -> its tuple on ``device``
        self._made = 0                   # epochs generated so far (they must be drawn in order)
        self.cursor = 0

    def _epoch(self, e):
        while self._made <= e:
            self._epochs[self._made] = tuple(None if t is None else t.to(self.device) for t in self._host_epoch())
            self._made += 1
        return self._epochs[e]

    def take(self, n, rank=0, world=1):
        """The epoch's tuple at positions [cursor + rank n, cursor + (rank + 1) n), each member [n]; the cursor moves by n world."""
        n = int(n)
        if n < 1:
            raise ValueError('a draw needs at least one %s' % self._what)
        start = self.cursor + rank * n
        self.cursor += n * world
        for e in [k for k in self._epochs if k < start // self._size]:          # epochs every rank has left behind
            del self._epochs[e]
        parts, pos = [], start
        while pos < start + n:
            e, off = divmod(pos, self._size)
            m = min(self._size - off, start + n - pos)
            parts.append(tuple(None if t is None else t[off:off + m] for t in self._epoch(e)))
            pos += m
        if self.device.type == 'cuda':
            s = torch.cuda.current_stream()
            for t in (t for p in parts for t in p if t is not None):
                t.record_stream(s)                                              # (read on this stream; freed when its epoch is over)
        if len(parts) == 1:
            return parts[0]
        return tuple(None if parts[0][k] is None else torch.cat([p[k] for p in parts]) for k in range(len(parts[0])))


class IndexStream(_EpochStream):
    """An endless sequence of image indices: ``torch.randperm(M, generator=g)`` per epoch, ``g`` a CPU generator seeded with ``seed``
    (the reference's InfiniteRandomSampler, train.py:51-56); ``arange(M)`` per epoch without ``shuffle``.  Mirror flags
    (``flags=True``) belong to positions too: ``torch.randint(0, 2, (M,), generator=g2, dtype=torch.uint8)`` per epoch, ``g2`` seeded
    ``seed + 1``.  ``take`` -> (idx [n] int64, flip [n] uint8 or None)."""

    def __init__(self, M, shuffle=True, seed=0, flags=False, device='cpu'):
        if int(M) < 1:
            raise ValueError('an index stream needs at least one image')
        super(IndexStream, self).__init__(M, 'image', shuffle, flags, device)
        self.M = int(M)
        self._g = torch.Generator().manual_seed(int(seed))
        self._g2 = torch.Generator().manual_seed(int(seed) + 1)

    def _host_epoch(self):
        idx = torch.randperm(self.M, generator=self._g) if self.shuffle else torch.arange(self.M)
        return idx, (torch.randint(0, 2, (self.M,), generator=self._g2, dtype=torch.uint8) if self.flags else None)


def _tiles(lengths, R):
    """(strip [P], start column [P]) int64 numpy arrays of the non-overlapping windows ``R`` columns wide of strips of ``lengths``
    columns, strip-major: item i of a strip dataset."""
    counts = np.asarray(lengths, dtype=np.int64) // R
    return np.repeat(np.arange(counts.size, dtype=np.int64), counts), np.concatenate([np.arange(c, dtype=np.int64) * R for c in counts])


class CropStream(_EpochStream):
    """An endless sequence of crops (strip, start column) from strips of ``lengths`` columns, windows ``R`` columns wide.  An epoch
    has P = sum(T_m // R) positions.  ``shuffle``: position by position, the strip is drawn with probability proportional to its
    number of window starts w_m = T_m - R + 1 -- p = min(floor(g W), W - 1), W = sum(w_m), strip = searchsorted(cumsum(w), p, right)
    -- and the start is t = min(floor(f w_m), w_m - 1): every start of every strip is equally likely.  g and f are float64 from
    ``torch.rand(P)`` on two CPU generators seeded ``seed`` and ``seed + 1``; the mirror flags (``flags=True``) are
    ``torch.randint(0, 2, (P,), dtype=torch.uint8)`` on a third seeded ``seed + 2``.  Without ``shuffle`` an epoch enumerates the
    non-overlapping windows (m, i R) in strip-major order.  ``t`` counts full-resolution columns, so the stream does not depend on
    the stage: at stored level k the start is t >> k, at most cols_k - (R >> k) when T_m and R are multiples of 2^k.
    ``take`` -> (idx [n] int64, pos [n] int64, flip [n] uint8 or None), with ``IndexStream``'s cursor rules."""

    def __init__(self, lengths, R, shuffle=True, seed=0, flags=False, device='cpu'):
        self.lengths, self.R = np.asarray([int(t) for t in lengths], dtype=np.int64), int(R)
        if self.lengths.size < 1 or int(self.lengths.min()) < self.R or self.R < 1:
            raise ValueError('a crop stream needs at least one strip, each of at least R = %d columns' % self.R)
        self.P = int((self.lengths // self.R).sum())
        super(CropStream, self).__init__(self.P, 'crop', shuffle, flags, device)
        self._g = [torch.Generator().manual_seed(int(seed) + k) for k in range(3)]
        self._w = self.lengths - self.R + 1
        self._cum = np.cumsum(self._w)

    def _draw(self):
        """(strip [P], start [P]) int64 numpy arrays of the next epoch."""
        if not self.shuffle:
            return _tiles(self.lengths, self.R)
        g = torch.rand(self.P, dtype=torch.float64, generator=self._g[0]).numpy()
        f = torch.rand(self.P, dtype=torch.float64, generator=self._g[1]).numpy()
        W = int(self._cum[-1])
        p = np.minimum(np.floor(g * W).astype(np.int64), W - 1)
        strip = np.searchsorted(self._cum, p, side='right').astype(np.int64)
        w = self._w[strip]
        return strip, np.minimum(np.floor(f * w).astype(np.int64), w - 1)

    def _host_epoch(self):
        strip, start = self._draw()
        flip = torch.randint(0, 2, (self.P,), generator=self._g[2], dtype=torch.uint8) if self.flags else None
        return torch.from_numpy(strip), torch.from_numpy(start), flip


def _log2(v):
    return int(v).bit_length() - 1


# ------------------------------------------------------------------------------------------------------- datasets
class _DeviceDataset(object):
    """What the two datasets share: N items [C,R,R] kept as uint8 levels on ``device``, the stage, one training stream and the batches.

    The stage is dataset depth ``model_depth + model_dataset_depth_offset`` (side 2^depth, so the default offset 2 starts at 4x4).
    ``pyramid`` picks which of the reference's two behaviours supplies a stage below the source resolution:

      'chain'   the ``preload=True`` pyramid (dataset.py:144-162): level k is made from level k + 1 with depth difference 1 -- a
                true 2x2 box mean, rounded to uint8 at EVERY level -- once, at construction, and kept (+1/3 memory); batches read the
                stage's level.
      'direct'  the ``preload=False`` path (dataset.py:201-203): nothing is stored, every batch is taken from the full-resolution
                level with depth difference log2(R) - depth, the reference's 4-SAMPLE SUBSAMPLING (the top-left 2x2 of every
                2^diff block).

    The two give different images for stages two or more levels below the source; they agree one level below and at the source.

    Protocol of the reference's DepthDataset: ``model_depth`` and ``alpha`` are plain attributes (DepthManager writes them),
    ``shape`` = (N,C,R,R), ``len()``, ``close()``, and ``dataset[i]`` = the reference's host tensor [C,r,r] fp32 of item i at the
    current depth and alpha (no mirror), so a plain ``DataLoader(dataset)`` still works.

    Batches: ``batch(n)`` -> fp32 [n,C,r,r] on ``device``, issued on the current stream; ``loader(n)`` -> endless iterator of
    them, what ``DepthManager(create_dataloader_fun=ds.loader, ...)`` takes; ``metric_batches()`` -> ``f(n)`` for
    ``SWDMonitor(real_batch_fn=...)``; ``items(idx)`` -> the batch of chosen items.  The training batches follow one stream whose
    cursor belongs to the dataset: a loader made at a stage change continues it, and the sequence does not depend on the batch sizes.
    ``mirror_augment`` flips images left-right by the stream's per-position flags.  Under data parallelism (``rank`` of ``world``, one
    seed everywhere) a draw of n takes positions [cursor + rank n, cursor + (rank + 1) n) and moves the cursor by n world: disjoint
    positions of one epoch.

    A subclass validates its ``source`` and gives ``_upload(source)`` (the full-resolution level), ``_level_below(level)``,
    ``_stream(seed, flags)``, ``_make(*drawn, alpha)`` for what its stream hands out, ``_locate(idx)`` (the leading members of such a
    tuple for items ``idx``), ``level_stack()`` and ``__getitem__``."""

    def __init__(self, source, shape, model_dataset_depth_offset, model_initial_depth, alpha, range_in, range_out, pyramid,
                 mirror_augment, shuffle, seed, rank, world, device):
        if pyramid not in ('chain', 'direct'):
            raise ValueError("pyramid must be 'chain' or 'direct', got %r" % (pyramid,))
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError('rank %r of world %r' % (rank, world))
        self.model_depth, self.alpha = model_initial_depth, alpha
        self.model_dataset_depth_offset = int(model_dataset_depth_offset)
        self.range_in, self.range_out = tuple(range_in), tuple(range_out)
        self.pyramid, self.mirror_augment, self.shuffle, self.seed = pyramid, bool(mirror_augment), bool(shuffle), int(seed)
        self.rank, self.world = int(rank), int(world)
        self.device = torch.device(device)
        self._shape = shape
        self.max_dataset_depth = _log2(shape[2])
        self.min_dataset_depth = self.max_dataset_depth if pyramid == 'direct' else min(self.max_dataset_depth, max(1, self.model_dataset_depth_offset))
        self._levels = {self.max_dataset_depth: self._upload(source)}
        for depth in range(self.max_dataset_depth - 1, self.min_dataset_depth - 1, -1):       # 'chain' only
            self._levels[depth] = self._level_below(self._levels[depth + 1])
        self._train = self._stream(self.seed, self.mirror_augment)

    # ------------------------------------------------------------------------------------------------- protocol
    @property
    def shape(self):
        return self._shape

    def __len__(self):
        return self._shape[0]

    def close(self):
        """Free the device buffers; the object is of no use afterwards."""
        self._levels = {}
        self._train = None

    def _stage(self):
        """(stored level to read, its levels below the source -- the shift of a start column --, depth difference left to the batch)
        of the current ``model_depth``."""
        if not self._levels:
            raise RuntimeError('the dataset is closed')
        depth = int(self.model_depth) + self.model_dataset_depth_offset
        lowest = self.min_dataset_depth if self.pyramid == 'chain' else 1
        if not lowest <= depth <= self.max_dataset_depth:
            raise ValueError('model_depth %r + offset %d is dataset depth %d; this dataset has depths %d .. %d'
                             % (self.model_depth, self.model_dataset_depth_offset, depth, lowest, self.max_dataset_depth))
        if self.pyramid == 'chain':
            return self._levels[depth], self.max_dataset_depth - depth, 0
        return self._levels[self.max_dataset_depth], 0, self.max_dataset_depth - depth

    # -------------------------------------------------------------------------------------------------- batches
    def _draw(self, n):
        if self._train is None:
            raise RuntimeError('the dataset is closed')
        return self._train.take(n, self.rank, self.world)

    @property
    def cursor(self):
        """Next unread position of the training stream (items drawn so far, over all ranks)."""
        return self._train.cursor

    def batch(self, n, alpha=None):
        """fp32 batch [n,C,r,r] at the current ``model_depth``, with ``self.alpha`` unless ``alpha`` is given, on the current stream."""
        return self._make(*self._draw(n), alpha=self.alpha if alpha is None else alpha)

    def loader(self, minibatch_size):
        """Endless iterator of ``batch(minibatch_size)``; every batch is drawn with the depth and alpha of that moment."""
        while True:
            yield self.batch(minibatch_size)

    def metric_batches(self, seed=1):
        """``f(n)`` -> fp32 batch [n,C,r,r] at the current ``model_depth`` with alpha = 1 and no mirror, from a stream and a
        cursor of its own (``f.stream``): evaluating a metric does not move the training stream."""
        stream = self._stream(seed, False)

        def real_batch_fn(n):
            return self._make(*stream.take(n), alpha=1.0)
        real_batch_fn.stream = stream
        return real_batch_fn

    def items(self, idx, alpha=1.0):
        """fp32 batch [n,C,r,r] of items ``idx`` (an int64 tensor [n] on ``device``, item i as in ``dataset[i]``) at the current
        ``model_depth``, no mirror; the training stream is not moved."""
        return self._make(*self._locate(idx), flip=None, alpha=alpha)


class DeviceImageDataset(_DeviceDataset):
    """``images``: uint8 numpy array or torch tensor [M,C,R,R], C in {1, 3}, R a power of two >= 4 (ValueError otherwise); at most
    ``max_images`` of them are used.  The stack is uploaded once (in chunks) and stays on ``device``.  ``two_channel=True`` announces
    C = 2, the 'magif' images of ``sound.spectrogram_stack_u8`` (log-magnitude and instantaneous frequency); unannounced, a
    two-channel stack stays the error it has always been (a sliced RGB stack).

    Stage, ``pyramid`` ('chain' levels are made with ``ops.pyramid_level_u8``), protocol and batches are ``_DeviceDataset``'s; item i
    is image i, the stream an ``IndexStream`` and a batch one launch of ``ops.real_batch_u8``.

    ``device='cpu'``: host mode, the same definition in numpy (fp64)."""

    def __init__(self, images, model_dataset_depth_offset=2, model_initial_depth=0, alpha=1.0, range_in=(0, 255), range_out=(-1, 1),
                 pyramid='chain', mirror_augment=False, shuffle=True, seed=0, max_images=None, rank=0, world=1, device='cuda', two_channel=False):
        if torch.is_tensor(images):
            ok = images.dtype == torch.uint8
        else:
            ok = isinstance(images, np.ndarray) and images.dtype == np.uint8
        if not ok:
            raise ValueError('images: expected a uint8 numpy array or torch tensor [M,C,R,R]')
        if images.ndim != 4 or images.shape[0] < 1:
            raise ValueError('images: expected [M,C,R,R] with M >= 1, got shape %s' % (tuple(images.shape),))
        M, C, R, R2 = (int(v) for v in images.shape)
        if C not in ((1, 2, 3) if two_channel else (1, 3)):
            raise ValueError('images: %d channels (1 or 3 are supported, 2 with two_channel=True)' % C)
        if R != R2 or R < 4 or R & (R - 1):
            raise ValueError('images: %dx%d (the side must be a power of two >= 4)' % (R, R2))
        if max_images is not None:
            if isinstance(max_images, bool) or int(max_images) != max_images or max_images < 1:
                raise ValueError('max_images must be None or a positive integer, got %r' % (max_images,))
            M = min(M, int(max_images))
        super(DeviceImageDataset, self).__init__(images, (M, C, R, R), model_dataset_depth_offset, model_initial_depth, alpha, range_in,
                                                 range_out, pyramid, mirror_augment, shuffle, seed, rank, world, device)

    # --------------------------------------------------------------------------------------------- construction
    @classmethod
    def from_npy(cls, path, **kw):
        """The stack of an ``.npy`` file [M,C,R,R] uint8, memory-mapped: only the chunk being uploaded is resident on the host."""
        return cls(np.load(path, mmap_mode='r'), **kw)

    @classmethod
    def from_folder(cls, dir_path, imread_mode='L', **kw):
        """Every file of ``dir_path`` in sorted order, read with PIL in ``imread_mode`` ('L', 'RGB') as the reference's ``load_file``
        reads it (dataset.py:229-236): [H,W] -> [1,H,W], [H,W,C] -> [C,H,W]."""
        import PIL.Image
        files = sorted(os.path.join(dir_path, f) for f in os.listdir(dir_path))
        if not files:
            raise ValueError('no files in %s' % dir_path)
        ims = []
        for f in files:
            im = np.asarray(PIL.Image.open(f).convert(imread_mode), dtype=np.uint8)
            ims.append(im[np.newaxis] if im.ndim == 2 else im.transpose(2, 0, 1))
            if ims[-1].shape != ims[0].shape:
                raise ValueError('%s is %s, %s is %s' % (files[0], ims[0].shape, f, ims[-1].shape))
        return cls(np.stack(ims), **kw)

    def _upload(self, images):
        M = len(self)
        if self.device.type != 'cuda':
            host = images[:M] if torch.is_tensor(images) else torch.from_numpy(np.array(images[:M]))
            return host.contiguous()
        from . import ops
        ops.require_gpu()
        per = int(np.prod(images.shape[1:]))
        step = max(1, UPLOAD_CHUNK_BYTES // per)
        dev = torch.empty((M,) + tuple(int(v) for v in images.shape[1:]), dtype=torch.uint8, device=self.device)
        for a in range(0, M, step):
            b = min(M, a + step)
            chunk = images[a:b] if torch.is_tensor(images) else torch.from_numpy(np.array(images[a:b]))      # (a copy: a memory-mapped file is read here)
            dev[a:b].copy_(chunk)
        return dev

    def _level_below(self, stack):
        if stack.is_cuda:
            from . import ops
            return ops.pyramid_level_u8(stack, 1, self.range_in)
        return torch.from_numpy(level_host(stack.numpy(), 1, self.range_in))

    def _stream(self, seed, flags):
        return IndexStream(len(self), self.shuffle, seed, flags=flags, device=self.device)

    # ------------------------------------------------------------------------------------------------- protocol
    def level_stack(self):
        """The uint8 stack [M,C,r,r] of the current ``model_depth``: what the batches of this stage are made from before fade-in, mirror
        and range (``metrics.NearestNeighbours`` searches it).  'chain': the stored level itself, no copy.  'direct': the stack itself at
        the source resolution; below it the level is made here, ``UPLOAD_CHUNK_BYTES`` of the stack at a time (``ops.pyramid_level_u8``
        on the device, ``level_host`` in host mode), and is NOT kept -- a caller that needs it repeatedly within a stage keeps it."""
        stack, _, dd = self._stage()
        if dd == 0:
            return stack
        M, C, R, _ = self._shape
        r = R >> dd
        out = torch.empty((M, C, r, r), dtype=torch.uint8, device=stack.device)
        step = max(1, UPLOAD_CHUNK_BYTES // (C * R * R))
        for a in range(0, M, step):
            b = min(M, a + step)
            if stack.is_cuda:
                from . import ops
                out[a:b].copy_(ops.pyramid_level_u8(stack[a:b], dd, self.range_in))
            else:
                out[a:b].copy_(torch.from_numpy(level_host(stack[a:b].numpy(), dd, self.range_in)))
        return out

    def __getitem__(self, item):
        i = int(item)
        if not -len(self) <= i < len(self):
            raise IndexError('image %d of %d' % (i, len(self)))
        stack, _, dd = self._stage()
        image = stack[i % len(self)].cpu().numpy()
        return torch.from_numpy(prepare_host(level_host(image, dd, self.range_in), self.alpha, self.range_in, self.range_out))

    # -------------------------------------------------------------------------------------------------- batches
    def _locate(self, idx):
        return (idx,)

    def _make(self, idx, flip, alpha):
        stack, _, dd = self._stage()
        if stack.is_cuda:
            from . import ops
            return ops.real_batch_u8(stack, idx, flip, dd, alpha, self.range_in, self.range_out)
        return torch.from_numpy(batch_host(stack.numpy(), idx.numpy(), None if flip is None else flip.numpy(), dd, alpha,
                                           self.range_in, self.range_out))

    def draw_indices(self, n):
        """The next ``n`` (image indices, mirror flags or None) of this rank from the training stream; moves the cursor."""
        return self._draw(n)


# ------------------------------------------------------------------------------------------- strips: random time-crops
def _pitch(cols):
    """Row pitch of a strip of ``cols`` columns: rounded up to the multiple include/pggan_hip_crop.h holds pitches and offsets to."""
    from ._lib import CROP_CONSTANTS
    align = CROP_CONSTANTS['PG_CROP_PITCH_ALIGN']
    return -(-int(cols) // align) * align


class StripLevel(object):
    """One stored level of a strip dataset on the device, what ``ops.crop_batch_u8`` reads: ``buffer``, ONE flat uint8 tensor with
    strip m laid out [C][S rows][pitch] at byte ``offset_m``, and ``table`` [M,3] int64 = (offset, pitch, columns) on the same device.
    Every pitch is the column count rounded up to 16 and every offset a multiple of 16; the padding bytes are zero and never reach
    a result.  ``cols`` and ``rows`` are the host's copies of the column counts and of the table."""

    def __init__(self, buffer, table, C, S, cols):
        self.buffer, self.table, self.C, self.S, self.cols = buffer, table, int(C), int(S), [int(c) for c in cols]
        self.rows = self.layout(self.C, self.S, self.cols)[0]             # the host's copy of the table

    @staticmethod
    def layout(C, S, cols):
        """(rows of (offset, pitch, columns), total bytes) of strips with ``cols`` columns."""
        rows, off = [], 0
        for c in cols:
            rows.append((off, _pitch(c), int(c)))
            off += C * S * _pitch(c)
        return rows, off

    @classmethod
    def empty(cls, C, S, cols, device):
        rows, total = cls.layout(C, S, cols)
        buffer = torch.zeros(total, dtype=torch.uint8, device=device)
        return cls(buffer, torch.tensor(rows, dtype=torch.int64).to(device), C, S, cols)

    @classmethod
    def pack(cls, strips, device):
        """The level of uint8 arrays or tensors [C,S,T_m] as they are (no truncation), each copied in one piece."""
        C, S = int(strips[0].shape[0]), int(strips[0].shape[1])
        level = cls.empty(C, S, [int(s.shape[2]) for s in strips], device)
        for m, s in enumerate(strips):
            level.strip(m).copy_(s if torch.is_tensor(s) else torch.from_numpy(np.ascontiguousarray(s)))
        return level

    def strip(self, m):
        """View [C, S, columns] of strip m (rows ``pitch`` bytes apart: not contiguous unless the pitch is the column count)."""
        off, pitch, cols = self.rows[m]
        return self.buffer[off:off + self.C * self.S * pitch].view(self.C, self.S, pitch)[:, :, :cols]

    @property
    def nbytes(self):
        return int(self.buffer.numel())


class DeviceStripDataset(_DeviceDataset):
    """Random time-crops of long recordings: ``strips`` is a list of uint8 numpy arrays or torch tensors [C, R, T_m] (spectrograms,
    time along the last axis), one C in {1, 2, 3} and one R (a power of two >= 4) for all of them, T_m >= R (ValueError otherwise,
    naming the strip).  Every strip is TRUNCATED to R (T_m // R) columns: then every pyramid level has whole columns and the
    non-overlapping windows tile every level.  A training image is the R x R window at a random start column t of a random strip
    (``CropStream``): all of every recording is used and every batch is a new translation.  Each strip is stored once, uint8, in HBM
    (``StripLevel``), and a batch -- gather of the windows where the strips lie, pyramid level, mirror, fade-in, dynamic range -- is
    one launch (``ops.crop_batch_u8``): nothing crosses PCIe and nothing synchronises per batch.

    Stage, ``pyramid``, protocol and batches are ``_DeviceDataset``'s.  k = log2(R) - depth levels below the source,

      'chain'   level k is made per strip (``ops.pyramid_level_u8``); a batch reads the window [t >> k, (t >> k) + r) of the stage's
                level, so a stage k levels down translates in steps of 2^k full-resolution columns.
      'direct'  a batch takes the window [t, t + R) of the full-resolution strip and subsamples it by depth difference k, at every
                start t.

    For windows that start at a multiple of R (``dataset[i]``, ``items``, ``level_stack()``, ``shuffle=False``) the two agree at the
    source and one level below, as for images.

    ``shape`` = (P, C, R, R) and ``len()`` = P = sum(T_m // R), the windows of an epoch; item i is NON-OVERLAPPING window i
    (strip-major).  ``level_stack()`` materialises the uint8 [P,C,r,r] stack of the non-overlapping windows of the current stage per
    call, so ``NNMonitor``, ``NDBMonitor`` and ``SWDMonitor(real_batch_fn=...)`` work unchanged.

    ``device='cpu'``: host mode, the numpy twin -- it slices the same windows and calls ``batch_host``."""

    def __init__(self, strips, model_dataset_depth_offset=2, model_initial_depth=0, alpha=1.0, range_in=(0, 255), range_out=(-1, 1),
                 pyramid='chain', mirror_augment=False, shuffle=True, seed=0, rank=0, world=1, device='cuda'):
        strips = list(strips)
        if not strips:
            raise ValueError('strips: expected at least one uint8 array [C,R,T]')
        for m, s in enumerate(strips):
            ok = s.dtype == torch.uint8 if torch.is_tensor(s) else isinstance(s, np.ndarray) and s.dtype == np.uint8
            if not ok or s.ndim != 3:
                raise ValueError('strip %d: expected a uint8 numpy array or torch tensor [C,R,T]' % m)
        C, R = int(strips[0].shape[0]), int(strips[0].shape[1])
        if C not in (1, 2, 3):
            raise ValueError('strip 0: %d channels (1, 2 or 3 are supported)' % C)
        if R < 4 or R & (R - 1):
            raise ValueError('strip 0: %d rows (the height must be a power of two >= 4)' % R)
        for m, s in enumerate(strips):
            if (int(s.shape[0]), int(s.shape[1])) != (C, R):
                raise ValueError('strip %d is [%d,%d,T], strip 0 is [%d,%d,T]' % (m, s.shape[0], s.shape[1], C, R))
            if int(s.shape[2]) < R:
                raise ValueError('strip %d: %d columns, a window needs %d' % (m, s.shape[2], R))
        self.lengths = [R * (int(s.shape[2]) // R) for s in strips]              # columns kept of every strip
        self._item_at = _tiles(self.lengths, R)                                  # item i -> (strip, start column), on the host ...
        super(DeviceStripDataset, self).__init__(strips, (len(self._item_at[0]), C, R, R), model_dataset_depth_offset, model_initial_depth,
                                                 alpha, range_in, range_out, pyramid, mirror_augment, shuffle, seed, rank, world, device)
        self._item_at_dev = tuple(torch.from_numpy(a).to(self.device) for a in self._item_at)      # ... and where ``items`` looks them up

    # --------------------------------------------------------------------------------------------- construction
    @classmethod
    def from_waveforms(cls, signals, n_fft=1024, hop_length=128, img_mode='magif', mag_range=None, sample_rate=None, mel_rows=None,
                       rates=None, frequency=None, **kw):
        """The dataset of a list of waveforms of different lengths (``[nsamp]`` or ``[nsamp, channels]``, numpy arrays or tensors):
        one strip per recording from ``sound.spectrogram_strip_u8``.  A waveform that gives fewer usable frames than the strip is
        high -- n_fft/2, or ``mel_rows`` for img_mode='melif', whose ``sample_rate`` and ``mel_rows`` are passed through -- is a
        ValueError naming it.

        ``rates`` and ``frequency`` (both or neither): the recordings' sample rates in Hz, one integer for all or one per waveform,
        and the rate every one of them is brought to by ``sound.resample`` before its analysis (SoundImageDataset's ``frequency``);
        the usable frames are those of the ``sound.resampled_length``."""
        from . import sound
        signals = list(signals)
        if (rates is None) != (frequency is None):
            raise ValueError('rates and frequency belong together: got rates %r and frequency %r' % (rates, frequency))
        if rates is None:
            rates = [None] * len(signals)                                       # (rate_in=None, frequency=None: no conversion)
        elif isinstance(rates, (int, np.integer)) and not isinstance(rates, bool):
            rates = [rates] * len(signals)
        try:
            rates = list(rates)
        except TypeError:
            raise ValueError('rates must be an integer or one per waveform, got %r' % (rates,))
        if len(rates) != len(signals):
            raise ValueError('rates: %d values for %d waveforms' % (len(rates), len(signals)))
        for rate in rates:                                                       # (positive integers; 'melif': sample_rate is the frequency)
            _, sample_rate = sound._resample_arguments(rate, frequency, img_mode, sample_rate)
        table = sound._mel_arguments(img_mode, n_fft, sample_rate, mel_rows)    # (refuses sample_rate / mel_rows with another mode first)
        side = int(n_fft) // 2 if table is None else table.rows
        strips = []
        for m, (y, rate) in enumerate(zip(signals, rates)):
            nsamp = int(y.shape[0]) if rate is None else sound.resampled_length(int(y.shape[0]), rate, frequency)
            if sound.strip_frames(nsamp, hop_length, img_mode) < side:
                converted = '' if rate is None else ' at %d Hz are %d samples at %d Hz and' % (rate, nsamp, frequency)
                raise ValueError('waveform %d: %d samples%s give %d usable frames, a window needs %d'
                                 % (m, y.shape[0], converted, sound.strip_frames(nsamp, hop_length, img_mode), side))
            strips.append(sound.spectrogram_strip_u8(y, n_fft, hop_length, img_mode, mag_range, sample_rate, mel_rows,
                                                     rate_in=rate, frequency=frequency))
        return cls(strips, **kw)

    @classmethod
    def from_wav_files(cls, paths, frequency=16000, **from_waveforms_kw):
        """The dataset of a list of WAV files of any sample rates: ``sound.load_wav`` per file (int16 samples go to the device as they
        are), then ``from_waveforms(rates=[the files' rates], frequency=frequency, **from_waveforms_kw)``.  A file that cannot be read
        is a ValueError naming it."""
        from . import sound
        loaded = [sound.load_wav(path) for path in paths]
        return cls.from_waveforms([y for _, y in loaded], rates=[rate for rate, _ in loaded], frequency=frequency, **from_waveforms_kw)

    def _upload(self, strips):
        """Host mode: a list of numpy arrays [C,R,T].  Device: a ``StripLevel``, filled ``UPLOAD_CHUNK_BYTES`` of columns at a time."""
        C, R = self._shape[1], self._shape[2]
        if self.device.type != 'cuda':
            return [np.ascontiguousarray((s.cpu().numpy() if torch.is_tensor(s) else s)[:, :, :t]) for s, t in zip(strips, self.lengths)]
        from . import ops
        ops.require_gpu()
        level = StripLevel.empty(C, R, self.lengths, self.device)
        step = max(1, UPLOAD_CHUNK_BYTES // (C * R))
        for m, (s, t) in enumerate(zip(strips, self.lengths)):
            dst = level.strip(m)
            for a in range(0, t, step):
                b = min(t, a + step)
                chunk = s[:, :, a:b] if torch.is_tensor(s) else torch.from_numpy(np.array(s[:, :, a:b]))   # (a copy: a memory-mapped file is read here)
                dst[:, :, a:b].copy_(chunk)
        return level

    def _level_below(self, level):
        if not isinstance(level, StripLevel):
            return [level_host(s, 1, self.range_in) for s in level]
        from . import ops
        below = StripLevel.empty(level.C, level.S // 2, [c // 2 for c in level.cols], self.device)
        for m in range(len(level.cols)):
            below.strip(m).copy_(ops.pyramid_level_u8(level.strip(m), 1, self.range_in))       # (takes H != W; makes the view contiguous)
        return below

    def _stream(self, seed, flags):
        return CropStream(self.lengths, self._shape[2], self.shuffle, seed, flags=flags, device=self.device)

    # ------------------------------------------------------------------------------------------------- protocol
    def level_bytes(self):
        """{dataset depth: bytes of its stored level} (device mode: the padded buffer; host mode: the arrays)."""
        return dict((d, lv.nbytes if isinstance(lv, StripLevel) else int(sum(s.nbytes for s in lv))) for d, lv in self._levels.items())

    @staticmethod
    def _strip_of(level, m):
        return level.strip(m) if isinstance(level, StripLevel) else level[m]

    def level_stack(self):
        """The uint8 stack [P,C,r,r] of the NON-OVERLAPPING windows of the current ``model_depth`` (strip-major), what
        ``metrics.NearestNeighbours`` and ``metrics.NDB`` search: materialised at every call and NOT kept -- a caller that needs it
        repeatedly within a stage keeps it.  'direct' below the source resolution makes the level of the windows here
        (``ops.pyramid_level_u8`` on the device, ``level_host`` in host mode)."""
        level, shift, dd = self._stage()
        P, C, R, _ = self._shape
        S = R >> shift
        parts = []
        for m in range(len(self.lengths)):
            s = self._strip_of(level, m)
            s = s if torch.is_tensor(s) else torch.from_numpy(s)
            parts.append(s.reshape(C, S, s.shape[2] // S, S).permute(2, 0, 1, 3))
        stack = torch.cat(parts).contiguous()
        if dd == 0:
            return stack
        if stack.is_cuda:
            from . import ops
            return ops.pyramid_level_u8(stack, dd, self.range_in)
        return torch.from_numpy(level_host(stack.numpy(), dd, self.range_in))

    def _windows_host(self, level, idx, pos, shift):
        """uint8 numpy stack [n,C,S,S] of the windows [pos >> shift, (pos >> shift) + S) of strips ``idx`` of a stored level."""
        S = self._shape[2] >> shift
        out = []
        for m, t in zip(np.asarray(idx).tolist(), np.asarray(pos).tolist()):
            s = self._strip_of(level, m)[:, :, (t >> shift):(t >> shift) + S]
            out.append(s.cpu().numpy() if torch.is_tensor(s) else s)
        return np.stack(out)

    def __getitem__(self, item):
        i = int(item)
        if not -len(self) <= i < len(self):
            raise IndexError('window %d of %d' % (i, len(self)))
        level, shift, dd = self._stage()
        window = self._windows_host(level, *(a[[i % len(self)]] for a in self._item_at), shift=shift)[0]
        return torch.from_numpy(prepare_host(level_host(window, dd, self.range_in), self.alpha, self.range_in, self.range_out))

    # -------------------------------------------------------------------------------------------------- batches
    def _locate(self, idx):
        return tuple(a[idx] for a in self._item_at_dev)

    def _make(self, idx, pos, flip, alpha):
        level, shift, dd = self._stage()
        if isinstance(level, StripLevel):
            from . import ops
            return ops.crop_batch_u8(level, idx, pos, flip, shift, dd, alpha, self.range_in, self.range_out)
        windows = self._windows_host(level, idx.numpy(), pos.numpy(), shift)
        return torch.from_numpy(batch_host(windows, np.arange(len(windows)), None if flip is None else flip.numpy(), dd, alpha,
                                           self.range_in, self.range_out))

    def draw_crops(self, n):
        """The next ``n`` (strips, start columns at full resolution, mirror flags or None) of this rank from the training stream;
        moves the cursor."""
        return self._draw(n)
