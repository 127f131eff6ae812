"""Quality metrics of a training run, evaluated on the device.

``SlicedWasserstein``: the sliced Wasserstein distance between Laplacian-pyramid patch descriptors of real and generated images
(Karras et al. 2018, "Progressive growing of GANs", section 5), one value per pyramid level -- one of the two metrics of the paper that need
no pretrained network (``MultiScaleSSIM`` below is the other).  The reference has no metric; the definition is the published one:

1. Laplacian pyramid of every image, levels ``R, R/2, ..., 16`` (``ops.lap_pyramid``);
2. per level, ``patches_per_image`` 3x7x7 neighbourhoods of every image as rows of 147 floats (``ops.swd_gather``);
3. per set and level, every channel normalised to zero mean and unit population standard deviation (``ops.swd_normalize_``);
4. ``dir_repeats`` times: project both sets on ``dirs_per_repeat`` unit directions, sort every projection, take the mean absolute
   difference of the sorted values (``ops.swd_project`` / ``swd_sort_rows_`` / ``swd_l1``); the value is the average x 1000.

``ChannelSlicedWasserstein`` is the same metric for networks with C = 1 .. 4 image channels -- the one-channel (``'abslog'``) and
two-channel (``'magif'``) spectrogram generators among them: descriptors are Cx7x7 = 49 C floats, every channel is normalised over the
whole set, directions are unit vectors of length 49 C (``ops.swd_gather_c`` / ``swd_normalize_c_`` / ``swd_project_c``).  For C != 3 it
is unpinned, this project's extension of the paper's 7x7x3 descriptor; with C = 3 it equals ``SlicedWasserstein`` bit for bit.

All randomness (patch centres, directions) comes from the object's own seeded CPU generator: the trainer's random stream is not touched
and the same seed gives the same metric.  The two sets use the SAME patch centres (image i of one set is sampled where image i of the
other is), so a set measured against itself gives exactly 0.

``MultiScaleSSIM``: the multi-scale structural similarity (Wang, Simoncelli & Bovik 2003) between pairs of GENERATED images, which
the paper uses to detect loss of variation: a generator that collapses onto a few images keeps a fair SWD for a while, but its
independent samples start to resemble each other and the mean MS-SSIM rises.  It is defined per channel, so one-channel (spectrogram)
networks are measured like RGB ones.  Definition: DESIGN.md section 7 (``ops.msssim_pairs``); it draws
no random numbers, so it has no seed.  Like the SWD it is UNPINNED: no vectors of the authors' implementation are at hand, the
values are comparable within a growth stage and between runs of this project.

``NearestNeighbours``: the nearest training images of generated samples by exact squared L2 distance over the 0..255 levels of the saved
image -- the paper's answer to "is that a new image or a copy of a training image?", which neither metric above can give (a generator
that memorises keeps a fine SWD, and MS-SSIM only sees collapse between samples).  Integer arithmetic: exact, the same from run to run.

``ShiftNearestNeighbours``: the same question for strip data sets, whose training images are windows at EVERY start column of long recordings:
the nearest window over all starts, segment by segment, without the per-start distances ever existing in memory.  Integer arithmetic as well.

``NDB``: the number of statistically different bins and the Jensen-Shannon divergence over k-means bins of the training images (Richardson &
Weiss 2018) -- does the generator cover the modes of the training set in the data's proportions, which none of the three above says.  Integer
k-means on the device-resident stack: exact and reproducible; UNPINNED like the SWD and MS-SSIM.

``PrecisionRecall``: improved precision and recall with density and coverage over k-NN balls in uint8 image space (Kynkaanniemi et al.
2019, Naeem et al. 2020) -- fidelity and coverage as separate numbers on one scale.  Three tile passes of exact integer distances of which
no distance is stored; UNPINNED as well.

``FrechetDistance``: the Frechet distance ``fd`` between the feature moments of the two sets over ``RandomEmbedding``, a randomly
initialised convolutional embedding (Naeem et al. 2020) -- the one metric here that is not in pixel space.  bf16 matrix cores for the
embedding, fp64 matrix cores for the moments, the statistic in fp64 on the host; reproducible from the seed; UNPINNED: it is not the
Inception distance and is not comparable with published FID tables.

``KernelDistance``: the kernel distance ``kid`` over the same embedding, the unbiased estimator of the squared maximum mean discrepancy
with a cubic polynomial kernel (Binkowski et al. 2018) -- unbiased at any sample count, where ``fd`` needs thousands of images a set.  The
kernel sums of 64 x 64 tiles on the fp64 matrix cores (no Gram matrix is written), the statistic in fp64 on the host; UNPINNED as well."""
import math

import numpy as np
import torch

from . import ops


def swd_levels(resolution):
    """Pyramid level sizes of a ``resolution`` x ``resolution`` image: resolution, resolution / 2, ..., 16."""
    resolution = int(resolution)
    if resolution < 16 or resolution & (resolution - 1):
        raise ValueError('resolution must be a power of two >= 16, got %r' % (resolution,))
    levels = []
    while resolution >= 16:
        levels.append(resolution)
        resolution //= 2
    return levels


def swd_draws(levels, rows, dir_repeats, width, dirs_per_repeat, seed):
    """The random part of the metric, from ONE CPU generator seeded ``seed``: first the patch centres (per level an int32 tensor
    ``[rows, 2]`` of (x, y) in [3, level - 4]), then the directions (fp32 ``[dir_repeats, width, dirs_per_repeat]``, unit columns,
    normalised in fp64).  The centres do not depend on ``width``."""
    gen = torch.Generator(device='cpu')
    gen.manual_seed(int(seed))
    centres = [torch.randint(3, s - 3, (rows, 2), generator=gen, dtype=torch.int32) for s in levels]
    for c, s in zip(centres, levels):                            # checked here, on the host, once: _feed gathers with check_range=False
        if int(c.min()) < 3 or int(c.max()) > s - 4:
            raise ValueError('patch centres outside [3, %d] at level %d' % (s - 4, s))
    d = torch.randn(dir_repeats, width, dirs_per_repeat, generator=gen, dtype=torch.float32).double()
    return centres, (d / d.pow(2).sum(dim=1, keepdim=True).sqrt()).float().contiguous()


class ChannelSlicedWasserstein(object):
    """Feed ``num_images`` real and as many generated fp32 ``[n,C,R,R]`` device batches (any split), then ``result()``;
    C = ``num_channels`` in 1 .. ``ops.SWD_MAX_CHANNELS``.  Unpinned for C != 3: this project's extension of the paper's 7x7x3
    descriptor.

    ``centres``: list (one per level) of int32 CPU tensors ``[num_images * patches_per_image, 2]`` of (x, y);
    ``directions``: fp32 CPU tensor ``[dir_repeats, 49 * C, dirs_per_repeat]`` with unit columns.  Centres, then directions, are
    drawn from one CPU generator seeded ``seed``: with ``num_channels=3`` they are ``SlicedWasserstein``'s of the same seed.
    ``phase_hook``: measurement aid (tools/swd_time.py), None by default; when set, ``hook(phase, fn, *args, **kw) -> fn(*args, **kw)``
    runs every ``ops`` call of an evaluation, ``phase`` one of ``PHASES``."""

    PHASES = ('pyramid', 'gather', 'normalise', 'project', 'sort', 'l1')
    _OPS = ('swd_gather_c', 'swd_normalize_c_', 'swd_project_c')          # names in ``ops`` of the three steps that see the channels

    def __init__(self, resolution, num_images, num_channels, patches_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=0,
                 device=None):
        self.levels = swd_levels(resolution)
        self.num_channels = self._channels(num_channels)
        self.desc_width = ops.SWD_PATCH * self.num_channels
        for name, v in (('num_images', num_images), ('patches_per_image', patches_per_image), ('dir_repeats', dir_repeats),
                        ('dirs_per_repeat', dirs_per_repeat)):
            if int(v) != v or v < 1:
                raise ValueError('%s must be a positive integer, got %r' % (name, v))
        self.resolution, self.num_images, self.patches = int(resolution), int(num_images), int(patches_per_image)
        self.dir_repeats, self.dirs_per_repeat, self.seed = int(dir_repeats), int(dirs_per_repeat), int(seed)
        self.rows = self.num_images * self.patches
        if self.rows > ops.SWD_SORT_MAX_M:
            raise ValueError('num_images * patches_per_image = %d descriptors per level; the sort takes at most %d'
                             % (self.rows, ops.SWD_SORT_MAX_M))
        self.centres, self.directions = swd_draws(self.levels, self.rows, self.dir_repeats, self.desc_width, self.dirs_per_repeat, self.seed)
        ops.require_gpu()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        dev = self.device
        self._centres_dev = [c.to(dev) for c in self.centres]
        self._dirs_dev = self.directions.to(dev)
        self._desc = {which: [torch.empty((self.rows, self.desc_width), device=dev, dtype=torch.float32) for _ in self.levels]
                      for which in ('real', 'fake')}
        # work buffers of ONE repeat: the two projected sets and the scratch of the merge passes
        shape = (self.dirs_per_repeat, self.rows)
        self._proj = [torch.empty(shape, device=dev, dtype=torch.float32) for _ in range(2)]
        self._tmp = torch.empty(shape, device=dev, dtype=torch.float32) if self.rows > ops.SWD_SORT_LDS_ROW else None
        self.phase_hook = None
        self.reset()

    @staticmethod
    def _channels(num_channels):
        return _int_in(num_channels, 1, ops.SWD_MAX_CHANNELS, 'num_channels must be an integer in 1 .. %d, got %r' % (ops.SWD_MAX_CHANNELS, num_channels))

    def _op(self, phase, fn, *args, **kw):
        return fn(*args, **kw) if self.phase_hook is None else self.phase_hook(phase, fn, *args, **kw)

    def reset(self):
        """Forget what was fed: the buffers are reused for the next evaluation."""
        self._fed = {'real': 0, 'fake': 0}
        self._result = None

    def _feed(self, which, batch):
        if not torch.is_tensor(batch) or batch.dim() != 4 \
                or tuple(batch.shape[1:]) != (self.num_channels, self.resolution, self.resolution):
            raise ValueError('expected a batch [n,%d,%d,%d], got %s' % (self.num_channels, self.resolution, self.resolution,
                                                                        tuple(batch.shape) if torch.is_tensor(batch) else type(batch)))
        n, fed = batch.shape[0], self._fed[which]
        if n < 1 or fed + n > self.num_images:
            raise ValueError('%d %s images fed, %d more would exceed num_images = %d' % (fed, which, n, self.num_images))
        if self._result is not None:
            raise RuntimeError('result() was taken: reset() before feeding again')
        P, gather = self.patches, getattr(ops, self._OPS[0])
        for li, level in enumerate(self._op('pyramid', ops.lap_pyramid, batch)):
            self._op('gather', gather, level, self._centres_dev[li][fed * P:(fed + n) * P], P, self._desc[which][li], fed * P,
                     check_range=False)
        self._fed[which] = fed + n

    def feed_real(self, batch):
        self._feed('real', batch)

    def feed_fake(self, batch):
        self._feed('fake', batch)

    @property
    def complete(self):
        return self._fed['real'] == self.num_images and self._fed['fake'] == self.num_images

    def result(self):
        """{'levels': [R, R/2, ..., 16], 'swd': [one value per level, x 1000], 'mean': their mean}.  One device synchronisation."""
        if self._result is None:
            if not self.complete:
                raise RuntimeError('fed %d real and %d fake images of %d' % (self._fed['real'], self._fed['fake'], self.num_images))
            dists = []
            normalize_, project = getattr(ops, self._OPS[1]), getattr(ops, self._OPS[2])
            for li in range(len(self.levels)):
                real, fake = self._desc['real'][li], self._desc['fake'][li]
                self._op('normalise', normalize_, real)
                self._op('normalise', normalize_, fake)
                for r in range(self.dir_repeats):
                    for desc, proj in ((real, self._proj[0]), (fake, self._proj[1])):
                        self._op('project', project, desc, self._dirs_dev[r], out=proj)
                        self._op('sort', ops.swd_sort_rows_, proj, self._tmp)
                    dists.append(self._op('l1', ops.swd_l1, self._proj[0], self._proj[1]))
            d = torch.stack(dists).cpu().double().view(len(self.levels), self.dir_repeats)
            swd = [float(v) for v in (d.mean(dim=1) * 1e3)]
            self._result = {'levels': list(self.levels), 'swd': swd, 'mean': sum(swd) / len(swd)}
        return self._result


class SlicedWasserstein(ChannelSlicedWasserstein):
    """The paper's form, three channels: feed ``num_images`` real and as many generated fp32 ``[n,3,R,R]`` device batches (any split),
    then ``result()``.  ``directions`` is ``[dir_repeats, 147, dirs_per_repeat]``; everything else is ``ChannelSlicedWasserstein``'s.
    Any other ``num_channels`` is refused here: ``ChannelSlicedWasserstein`` takes 1 .. 4."""

    _OPS = ('swd_gather', 'swd_normalize_', 'swd_project')

    def __init__(self, resolution, num_images, patches_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=0, num_channels=3,
                 device=None):
        super(SlicedWasserstein, self).__init__(resolution, num_images, num_channels, patches_per_image=patches_per_image,
                                                dir_repeats=dir_repeats, dirs_per_repeat=dirs_per_repeat, seed=seed, device=device)

    @staticmethod
    def _channels(num_channels):
        if int(num_channels) != 3:
            raise ValueError('the descriptors are 3x7x7: single-channel (or any non-RGB) networks are out of contract')
        return 3


class MultiScaleSSIM(object):
    """Feed ``num_pairs`` pairs of fp32 device batches ``a, b [n,C,R,R]`` (any split; pair i is ``(a[i], b[i])``), then ``result()``.

    ``quantize``: measure the 0..255 levels of the saved image (``drange`` mapped, rounded half to even, clipped), the default;
    False maps the range only.  Scratch is the pooled images and partial sums of ONE fed batch, allocated at the first ``feed`` for
    that batch size (a larger batch later re-allocates) and reused."""

    def __init__(self, resolution, num_pairs, num_channels=3, drange=(-1, 1), quantize=True, device=None):
        self.scales, self.weights = ops.msssim_scales(resolution)
        if int(num_channels) not in (1, 3):
            raise ValueError('num_channels must be 1 or 3, got %r' % (num_channels,))
        if int(num_pairs) != num_pairs or num_pairs < 1:
            raise ValueError('num_pairs must be a positive integer, got %r' % (num_pairs,))
        if not float(drange[1]) > float(drange[0]):
            raise ValueError('drange must be (lo, hi) with hi > lo, got %r' % (drange,))
        self.resolution, self.num_pairs, self.num_channels = int(resolution), int(num_pairs), int(num_channels)
        self.drange, self.quantize = (float(drange[0]), float(drange[1])), bool(quantize)
        ops.require_gpu()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._values = torch.empty(self.num_pairs, device=self.device, dtype=torch.float64)
        self._terms = torch.empty((self.num_pairs, len(self.scales)), device=self.device, dtype=torch.float64)
        self._scratch = None
        self.reset()

    def reset(self):
        """Forget what was fed: the buffers are reused for the next evaluation."""
        self._fed = 0
        self._result = None

    def feed(self, a, b):
        shape = (self.num_channels, self.resolution, self.resolution)
        for t in (a, b):
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[1:]) != shape:
                raise ValueError('expected batches [n,%d,%d,%d], got %s' % (shape + (tuple(t.shape) if torch.is_tensor(t) else type(t),)))
        if self._result is not None:                                        # (before the count: a finished evaluation is full by definition)
            raise RuntimeError('result() was taken: reset() before feeding again')
        n, fed = a.shape[0], self._fed
        if n < 1 or fed + n > self.num_pairs:
            raise ValueError('%d pairs fed, %d more would exceed num_pairs = %d' % (fed, n, self.num_pairs))
        if self._scratch is None or self._scratch.n < n:
            self._scratch = None
            self._scratch = ops.MSSSIMScratch(n, self.num_channels, self.resolution, self.device)
        ops.msssim_pairs(a, b, self.drange, self.quantize, out=(self._values[fed:fed + n], self._terms[fed:fed + n]),
                         scratch=self._scratch)
        self._fed = fed + n

    @property
    def complete(self):
        return self._fed == self.num_pairs

    def result(self):
        """{'msssim': mean over the pairs, 'std': their population standard deviation, 'scales': [R, R/2, ...], 'terms': the mean of
        every scale's term (contrast-structure below the last scale, ssim at the last)}, in fp64 on the host.  One device synchronisation."""
        if self._result is None:
            if not self.complete:
                raise RuntimeError('fed %d pairs of %d' % (self._fed, self.num_pairs))
            both = torch.cat([self._values.view(-1, 1), self._terms], dim=1).cpu()
            v = both[:, 0]
            mean = float(v.mean())
            self._result = {'msssim': mean, 'std': float((v - mean).pow(2).mean().sqrt()), 'scales': list(self.scales),
                            'terms': [float(t) for t in both[:, 1:].mean(dim=0)]}
        return self._result


def _quantise_host(x, drange):
    """``ops.quantize_u8`` in numpy float32: one rounding per operation, round half to even, clip."""
    lo, hi = float(drange[0]), float(drange[1])
    y = (np.asarray(x, dtype=np.float32) - np.float32(lo)) * np.float32(255.0 / (hi - lo))
    return np.clip(np.round(y), 0, 255).astype(np.uint8)


def _int_in(v, lo, hi, message):
    """``int(v)`` of an integer (a bool is none) with lo <= v <= hi (None: no bound on that side), else ``ValueError(message)``."""
    if isinstance(v, bool) or int(v) != v or (lo is not None and v < lo) or (hi is not None and v > hi):
        raise ValueError(message)
    return int(v)


class _LevelMetric(object):
    """What the metrics over the 0..255 levels of the saved image share (``NearestNeighbours``, ``ShiftNearestNeighbours``, ``NDB``,
    ``PrecisionRecall``): ``drange`` and the ``device`` rule (None = where the source is, 'cpu' = the numpy twin), the one place that
    quantises samples (``_levels``), the sample check and the host merge of a mirrored search.  A new metric states its own source
    and arguments, then calls ``__init__`` here."""

    def __init__(self, source, src_device, drange, device):
        if not float(drange[1]) > float(drange[0]):
            raise ValueError('drange must be (lo, hi) with hi > lo, got %r' % (drange,))
        self.source, self.drange = source, (float(drange[0]), float(drange[1]))
        self.device = torch.device(src_device if device is None else device)

    @staticmethod
    def _check_range_in(source):
        if tuple(source.range_in) != (0, 255):
            raise ValueError('source: the data set holds range_in = %r; the metric compares 0..255 levels' % (tuple(source.range_in),))

    def _levels(self, samples, mirror=False):
        """fp32 samples in ``drange`` -> their uint8 levels on ``device`` (``ops.quantize_u8``, or its numpy twin in host mode);
        ``mirror``: followed by the left-right flipped copies."""
        if self.device.type == 'cuda':
            q = ops.quantize_u8(samples.to(self.device).contiguous(), self.drange)
        else:
            q = torch.from_numpy(_quantise_host(samples.cpu().numpy(), self.drange))
        return torch.cat([q, q.flip(-1)]) if mirror else q

    @staticmethod
    def _check_samples(samples, shape):
        if not torch.is_tensor(samples) or samples.dtype != torch.float32 or samples.dim() != 4 or samples.shape[0] < 1 \
                or tuple(samples.shape[1:]) != tuple(shape):
            raise ValueError('expected float32 samples [K,%d,%d,%d], got %s'
                             % (tuple(shape) + (tuple(samples.shape) if torch.is_tensor(samples) else type(samples),)))

    @staticmethod
    def _merge_mirrored(*columns):
        """The two sorted lists of k per sample of a mirrored search -> the k smallest keys of both.  ``columns``: arrays [2 K, k] in
        KEY ORDER (most significant first), rows K .. 2 K - 1 the mirrored queries'; ``mirrored`` is the last, least significant key.
        Returns the merged columns [K, k] and ``mirrored`` bool [K, k]."""
        K, k = columns[0].shape[0] // 2, columns[0].shape[1]
        both = [np.concatenate([a[:K], a[K:]], axis=1) for a in columns]
        both.append(np.concatenate([np.zeros((K, k), dtype=bool), np.ones((K, k), dtype=bool)], axis=1))
        order = np.stack([np.lexsort([a[i] for a in reversed(both)])[:k] for i in range(K)])      # (lexsort: the LAST key is primary)
        return [np.take_along_axis(a, order, axis=1) for a in both]


class _StackSource(object):
    """The source of the metrics over an image stack: a uint8 tensor [M,C,r,r] or a data set with ``level_stack()``."""

    @staticmethod
    def _stack_source(source):
        """(M, device) of a valid source."""
        if torch.is_tensor(source):
            if source.dtype != torch.uint8 or source.dim() != 4 or source.shape[0] < 1:
                raise ValueError('source: expected a device dataset or a uint8 tensor [M,C,r,r]')
            return source.shape[0], source.device
        if not hasattr(source, 'level_stack'):
            raise ValueError('source: expected a device dataset or a uint8 tensor [M,C,r,r], got %s' % type(source))
        _LevelMetric._check_range_in(source)
        return len(source), source.device

    def stack(self):
        """The uint8 stack [M,C,r,r] a search or a fit made now would read, on ``device``."""
        s = self.source if torch.is_tensor(self.source) else self.source.level_stack()
        return s if s.device == self.device else s.to(self.device)


class _FittedFeed(object):
    """The feed of the metrics that are fitted on the training stack once per stage and then fed generated images (``NDB``,
    ``PrecisionRecall``, ``FrechetDistance``).  The class supplies ``fit()`` -- which sets ``shape``, the [C,r,r] of the fitted stage -- ``reset()`` --
    which zeroes ``_fed`` and ``_result`` -- ``_take(images_u8)``, what it does with a checked uint8 batch on ``device``, and
    ``result()``."""

    def _fitted(self, images, dtype, what):
        if self.shape is None:
            raise RuntimeError('fit() first')
        if not torch.is_tensor(images) or images.dtype != dtype or images.dim() != 4 or images.shape[0] < 1 \
                or tuple(images.shape[1:]) != self.shape:
            raise ValueError('%s: expected %s images [n,%d,%d,%d] (the fitted stage), got %s'
                             % ((what, str(dtype).replace('torch.', '')) + self.shape
                                + (tuple(images.shape) if torch.is_tensor(images) else type(images),)))
        if self._result is not None:
            raise RuntimeError('result() was taken: reset() before feeding again')

    def feed(self, samples):
        """Generated fp32 images [n,C,r,r] in ``drange``, n >= 1."""
        self._fitted(samples, torch.float32, 'feed')
        self.feed_u8(self._levels(samples))

    def feed_u8(self, images):
        """Generated images as 0..255 levels, uint8 [n,C,r,r], n >= 1."""
        self._fitted(images, torch.uint8, 'feed_u8')
        self._take(images.to(self.device))
        self._fed += images.shape[0]


def _search_host(stack, queries, k):
    """``ops.nn_search_u8`` in numpy int64: (sqdist [K,k], index [K,k]), ascending by (distance, index)."""
    M = stack.shape[0]
    x = stack.reshape(M, -1).astype(np.int32)
    sq, ix = [], []
    for q in queries.reshape(queries.shape[0], -1).astype(np.int32):
        d = x - q[None]
        dist = (d * d).sum(axis=1, dtype=np.int64)                     # (a difference squared is at most 65025)
        order = np.lexsort((np.arange(M), dist))[:k]
        sq.append(dist[order])
        ix.append(order)
    return np.stack(sq).astype(np.int64), np.stack(ix).astype(np.int64)


class NearestNeighbours(_StackSource, _LevelMetric):
    """``search(samples)``: the ``k`` nearest training images of every generated sample.

    ``source``: a ``DeviceImageDataset`` -- the stack of its current ``model_depth`` is taken at every call (``level_stack()``), so the
    search follows the growth stage; its ``range_in`` must be (0, 255) -- or a uint8 tensor [M,C,r,r].  The samples (fp32 [K,C,r,r] in
    ``drange``) are rounded to the 0..255 levels of the saved image (``ops.quantize_u8``) and compared byte for byte with the stack:
    ``sqdist = sum_d (x_d - q_d)^2``, exact (``ops.nn_search_u8``: one pass over the stack per ``ops.NN_MAX_QUERIES`` queries), neighbours
    ascending by (sqdist, index).  ``mirror``: also compare every sample's left-right mirror image (the queries are doubled with their
    flipped copies) and merge the two lists of a sample on the host by (sqdist, index, mirrored) -- for a data set trained with
    ``mirror_augment`` a mirrored training image is a training image.  1 <= k <= min(M, ops.NN_MAX_TOPK).

    ``device``: None = where the source is; 'cpu' = the numpy twin in int64 (the same definition, no device)."""

    def __init__(self, source, k=1, mirror=False, drange=(-1, 1), device=None):
        M, src_device = self._stack_source(source)
        self.k = _int_in(k, 1, min(M, ops.NN_MAX_TOPK), 'k = %r for %d images (1 <= k <= min(M, %d))' % (k, M, ops.NN_MAX_TOPK))
        self.mirror = bool(mirror)
        super(NearestNeighbours, self).__init__(source, src_device, drange, device)

    def search(self, samples):
        """{'index': int64 [K,k], 'sqdist': int64 [K,k], 'rms': float64 [K,k] = sqrt(sqdist / D) in 0..255 levels (fp64, host),
        'mirrored': bool [K,k] (the neighbour matches the sample's mirror image)} as host tensors.  One device synchronisation."""
        stack = self.stack()
        self._check_samples(samples, stack.shape[1:])
        K, k = samples.shape[0], self.k
        q = self._levels(samples, self.mirror)
        if self.device.type == 'cuda':
            sq, ix = torch.stack(ops.nn_search_u8(stack.contiguous(), q, k)).cpu().numpy()
        else:
            sq, ix = _search_host(stack.numpy(), q.numpy(), k)
        sq, ix, mirrored = self._merge_mirrored(sq, ix) if self.mirror else (sq, ix, np.zeros((K, k), dtype=bool))
        D = int(np.prod(stack.shape[1:]))
        return {'index': torch.from_numpy(np.ascontiguousarray(ix)), 'sqdist': torch.from_numpy(np.ascontiguousarray(sq)),
                'rms': torch.from_numpy(np.sqrt(sq.astype(np.float64) / D)), 'mirrored': torch.from_numpy(np.ascontiguousarray(mirrored))}

    def neighbours(self, result):
        """The images a ``search`` result names: fp32 [K,k,C,r,r] in ``drange`` on ``device``, mirrored where the result says so
        (``ops.real_batch_u8`` with alpha 1)."""
        stack = self.stack()
        idx, flip = result['index'].reshape(-1), result['mirrored'].reshape(-1).to(torch.uint8)
        if self.device.type == 'cuda':
            out = ops.real_batch_u8(stack.contiguous(), idx.to(self.device), flip.to(self.device), 0, 1.0, (0, 255), self.drange)
        else:
            from .dataset import batch_host
            out = torch.from_numpy(batch_host(stack.numpy(), idx.numpy(), flip.numpy(), 0, 1.0, (0, 255), self.drange))
        return out.view(tuple(result['index'].shape) + tuple(stack.shape[1:]))


# ------------------------------------------------------------------------- nearest windows at every start column of strips
def _shift_keys_host(strips, queries, seg):
    """``ops.shift_l2min_u8`` in numpy int64: ``strips`` a list of uint8 arrays [C,S,T_m], ``queries`` uint8 [K,C,S,S] -> keys [K,G].
    The distances of one strip at all starts are accumulated column by column of the query (never as materialised windows)."""
    K, C, S, _ = queries.shape
    q = queries.astype(np.int64)
    keys = []
    for s in strips:
        n = s.shape[2] - S + 1
        x = np.asarray(s).astype(np.int64)
        d = np.zeros((K, n), dtype=np.int64)
        for j in range(S):
            diff = x[None, :, :, j:j + n] - q[:, :, :, j, None]              # [K,C,S,n]: column j of every query against columns j + u
            d += (diff * diff).sum(axis=(1, 2))
        for g0 in range(0, n, seg):
            part = (d[:, g0:g0 + seg] << ops.SHIFT_POS_BITS) + np.arange(min(seg, n - g0), dtype=np.int64)[None]
            keys.append(part.min(axis=1))
    return np.stack(keys, axis=1)


def _topk_host(keys, k):
    """``ops.topk_smallest_i64`` in numpy: (values [K,k], indices [K,k]), ascending by (value, index)."""
    order = np.stack([np.lexsort((np.arange(row.size), row))[:k] for row in keys])
    return np.take_along_axis(keys, order, axis=1), order.astype(np.int64)


class ShiftNearestNeighbours(_LevelMetric):
    """``search(samples)``: the ``k`` nearest training WINDOWS of every generated sample over every start column of the recordings --
    what ``NearestNeighbours`` on ``level_stack()`` cannot see, because that stack holds only the windows whose start is a multiple
    of the window width.

    ``source``: a ``DeviceStripDataset`` (its ``range_in`` must be (0, 255)) or a ``dataset.StripLevel``.  With a data set the search
    follows the growth stage (``_stage()``): for ``pyramid='chain'`` the stage's stored level is searched with windows S = R >> shift
    at every STORED column, so a reported start is ``u << shift`` full-resolution columns; for ``'direct'`` below the source resolution
    a level is made per strip with ``ops.pyramid_level_u8(strip, dd)``, once per stage and kept until the stage moves, which gives
    the translations that are multiples of 2^dd full-resolution columns (the training crops of 'direct' start at every column: the
    others are not searched).

    The samples (fp32 [K,C,S,S] in ``drange``) are rounded to the 0..255 levels (``ops.quantize_u8``) and compared byte for byte:
    ``sqdist = sum (x - q)^2`` exact.  The starts of every strip are cut into segments of ``seg`` starts (default S;
    ``ops.shift_segments``); ``ops.shift_l2min_u8`` gives the nearest start of every segment and ``ops.topk_smallest_i64`` the ``k``
    nearest SEGMENTS, ascending by (sqdist, start within the segment, segment).  One neighbour per segment: two adjacent segments may
    report nearly the same place (starts seg - 1 and seg are one column apart); that is accepted, not suppressed.  The distances of
    the individual starts never exist in memory.  ``mirror``: the queries are doubled with their time-reversed copies and the two
    lists of a sample merged on the host by (sqdist, segment, start, mirrored).  1 <= k <= min(G, ops.NN_MAX_TOPK).

    ``device``: None = where the source is; 'cpu' = the numpy twin in int64 (the same definition, no device)."""

    def __init__(self, source, k=1, mirror=False, drange=(-1, 1), seg=None, device=None):
        from .dataset import StripLevel
        if isinstance(source, StripLevel):
            src_device, S, cols = source.buffer.device, source.S, source.cols
        elif hasattr(source, '_stage') and hasattr(source, 'lengths'):
            self._check_range_in(source)
            src_device, S, cols = source.device, source.shape[2], source.lengths
        else:
            raise ValueError('source: expected a DeviceStripDataset or a StripLevel, got %s' % type(source))
        if seg is not None:
            ops._shift_seg(S, seg)
        G = len(ops.shift_segments(cols, S, seg)[0])                     # (the same at every stage when seg is None: T and S shrink together)
        self.k = _int_in(k, 1, min(G, ops.NN_MAX_TOPK), 'k = %r for %d segments (1 <= k <= min(G, %d))' % (k, G, ops.NN_MAX_TOPK))
        self.mirror, self.seg = bool(mirror), None if seg is None else int(seg)
        super(ShiftNearestNeighbours, self).__init__(source, src_device, drange, device)
        self._made = (None, None)                                        # ('direct' below the source: (stage key, the level made for it))

    # ------------------------------------------------------------------------------------------------- the level
    def level(self):
        """(the level a search made now would read, log2 of the full-resolution columns per column of it): a ``StripLevel`` on the
        device, a list of uint8 numpy arrays [C,S,T] in host mode."""
        from .dataset import StripLevel, level_host
        if isinstance(self.source, StripLevel):
            level, shift, dd = self.source, 0, 0
        else:
            level, shift, dd = self.source._stage()
        host = self.device.type != 'cuda'
        if dd == 0 and host == (not isinstance(level, StripLevel)):
            return level, shift
        key = (id(level), dd, host)
        if self._made[0] != key:
            self._made = (None, None)                                    # (drop the last stage's before making this one's)
            M = len(level.cols) if isinstance(level, StripLevel) else len(level)
            strips = [level.strip(m) if isinstance(level, StripLevel) else level[m] for m in range(M)]
            if host:
                strips = [s.cpu().numpy() if torch.is_tensor(s) else s for s in strips]
                made = [level_host(s, dd, self.source.range_in) for s in strips] if dd else strips
            else:
                made = StripLevel.pack([ops.pyramid_level_u8(s if torch.is_tensor(s) else torch.from_numpy(s).to(self.device), dd,
                                                             self.source.range_in) for s in strips], self.device)
            self._made = (key, made)
        return self._made[1], shift + dd

    @staticmethod
    def _dims(level):
        """(C, S, columns per strip) of a device or host level."""
        if isinstance(level, list):
            return level[0].shape[0], level[0].shape[1], [s.shape[2] for s in level]
        return level.C, level.S, level.cols

    def _seg(self, S):
        return ops._shift_seg(S, self.seg)[1]

    # ------------------------------------------------------------------------------------------------ the search
    def search(self, samples):
        """{'strip': int64 [K,k], 'start': int64 [K,k] (full-resolution start column of the window), 'sqdist': int64 [K,k],
        'rms': float64 [K,k] = sqrt(sqdist / D) in 0..255 levels (fp64, host), 'mirrored': bool [K,k] (the window matches the sample
        reversed in time)} as host tensors.  One device synchronisation."""
        level, scale = self.level()
        C, S, cols = self._dims(level)
        self._check_samples(samples, (C, S, S))
        seg = self._seg(S)
        seg_strip, seg_start, _ = ops.shift_segments(cols, S, seg)
        K, k = samples.shape[0], self.k
        if k > seg_strip.size:
            raise ValueError('k = %d for %d segments at this stage' % (k, seg_strip.size))
        q = self._levels(samples, self.mirror)
        if self.device.type == 'cuda':
            val, ix = torch.stack(ops.topk_smallest_i64(ops.shift_l2min_u8(level, q, seg), k)).cpu().numpy()
        else:
            val, ix = _topk_host(_shift_keys_host(level, q.numpy(), seg), k)
        sq, off = val >> ops.SHIFT_POS_BITS, val & (ops.SHIFT_MAX_SEG - 1)
        sq, ix, off, mirrored = self._merge_mirrored(sq, ix, off) if self.mirror else (sq, ix, off, np.zeros((K, k), dtype=bool))
        D = C * S * S
        start = (seg_start[ix] + off) << scale
        return {'strip': torch.from_numpy(np.ascontiguousarray(seg_strip[ix])), 'start': torch.from_numpy(np.ascontiguousarray(start)),
                'sqdist': torch.from_numpy(np.ascontiguousarray(sq)), 'rms': torch.from_numpy(np.sqrt(sq.astype(np.float64) / D)),
                'mirrored': torch.from_numpy(np.ascontiguousarray(mirrored))}

    def neighbours(self, result):
        """The windows a ``search`` result names: fp32 [K,k,C,S,S] in ``drange`` on ``device``, reversed in time where the result says
        so (``ops.crop_batch_u8`` with alpha 1)."""
        level, scale = self.level()
        C, S, _ = self._dims(level)
        idx, pos = result['strip'].reshape(-1).contiguous(), result['start'].reshape(-1).contiguous()
        flip = result['mirrored'].reshape(-1).to(torch.uint8).contiguous()
        if self.device.type == 'cuda':
            out = ops.crop_batch_u8(level, idx.to(self.device), pos.to(self.device), flip.to(self.device), scale, 0, 1.0, (0, 255), self.drange)
        else:
            from .dataset import batch_host
            windows = np.stack([level[m][:, :, (t >> scale):(t >> scale) + S] for m, t in zip(idx.tolist(), pos.tolist())])
            out = torch.from_numpy(batch_host(windows, np.arange(len(windows)), flip.numpy(), 0, 1.0, (0, 255), self.drange))
        return out.view(tuple(result['strip'].shape) + (C, S, S))


# ------------------------------------------------------------------------------------------------ NDB/k and JSD (k-means bins)
Z_THRESHOLD_05 = 1.959963984540054                 # two-sided alpha = 0.05 of the standard normal: Phi^-1(0.975)


def _d2_host(a, b):
    """int64 [Na,Nb]: the exact squared L2 distances between the rows of two uint8 arrays [n,D]."""
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    return (a64 * a64).sum(axis=1)[:, None] - 2 * (a64 @ b64.T) + (b64 * b64).sum(axis=1)[None]


def _assign_host(x, c):
    """``cluster.assign_u8`` in numpy int64: x [M,D], c [K,D] uint8 -> (label int32 [M], sqdist int64 [M]); argmin takes the first
    (lowest k) of equal distances."""
    dist = _d2_host(x, c)
    label = dist.argmin(axis=1)
    return label.astype(np.int32), dist[np.arange(x.shape[0]), label]


def _update_host(x, label, c):
    """``cluster.cluster_sums_u8`` + ``centroids_u8`` in numpy int64: label -1 is no member; an empty bin keeps its centroid."""
    K = c.shape[0]
    member = label >= 0
    counts = np.bincount(label[member], minlength=K).astype(np.int64)
    sums = np.zeros(c.shape, dtype=np.int64)
    np.add.at(sums, label[member], x[member].astype(np.int64))
    new = c.copy()
    filled = counts > 0
    n = counts[filled][:, None]
    new[filled] = ((2 * sums[filled] + n) // (2 * n)).astype(np.uint8)
    return new


def ndb_statistic(ref, gen, z_threshold=Z_THRESHOLD_05):
    """The two-sample test per bin and the JS divergence of the two histograms, in fp64 on the host: ``ref``,
    ``gen`` integer counts [K] -> {'ndb', 'ndb_over_k', 'jsd', 'z'}.  A bin whose standard error is 0 has z = 0."""
    ref, gen = np.asarray(ref, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    P, Q = ref.sum(), gen.sum()
    if not (P > 0 and Q > 0):
        raise ValueError('both histograms need at least one sample')
    p, q, pool = ref / P, gen / Q, (ref + gen) / (P + Q)
    se = np.sqrt(pool * (1.0 - pool) * (1.0 / P + 1.0 / Q))
    z = np.zeros_like(p)
    np.divide(p - q, se, out=z, where=se > 0)
    ndb = int((np.abs(z) > z_threshold).sum())
    m = 0.5 * (p + q)
    # K <= 64 terms, added in ascending k on Python floats: the order is part of the definition's bits (0 log 0 = 0)
    kl_p = sum(float(a) * math.log2(float(a) / float(b)) for a, b in zip(p, m) if a > 0)
    kl_q = sum(float(a) * math.log2(float(a) / float(b)) for a, b in zip(q, m) if a > 0)
    return {'ndb': ndb, 'ndb_over_k': ndb / float(len(ref)), 'jsd': 0.5 * kl_p + 0.5 * kl_q, 'z': z}


class NDB(_StackSource, _FittedFeed, _LevelMetric):
    """Number of statistically different bins (NDB/k) and the Jensen-Shannon divergence of the bin histograms (Richardson & Weiss 2018,
    "On GANs and GMMs"): does the generator cover the modes of the training set in the data's proportions?  ``fit()`` clusters the
    training images into ``k`` Voronoi cells by k-means in pixel space; ``feed`` counts generated images per cell; ``result()`` counts the
    cells whose share of generated images differs from their share of training images by a two-sample test, and the JSD of the two
    histograms.  Defined per image vector: one-channel networks are measured like RGB ones.

    ``source``: a ``DeviceImageDataset`` (``fit()`` takes ``level_stack()`` of its current ``model_depth``; ``range_in`` must be
    (0, 255)) or a uint8 tensor [M,C,r,r]; D = C r^2 a multiple of 16, M <= ``cluster.MAX_IMAGES``, 2 <= k <= ``ops.NN_MAX_QUERIES``.
    ``holdout`` = h, 0 <= h < M - k + 1: the first h entries of ``torch.randperm(M)`` from a CPU generator seeded ``seed`` are held out
    of the fit and the reference proportions are counted on THEM; h = 0 is the paper's form (reference proportions on the fitted images
    themselves), under which a fresh sample of the SAME distribution already differs in many bins -- a centroid is nearer to its own
    members than to new points -- so a hold-out is the form to use.  The initial centroids are copies of the first k images of a
    second permutation, of the fit set, seeded ``seed + 1``.  An iteration assigns ALL images (``label = argmin_k`` of the exact
    squared distance, the lower k of equal ones) and moves every centroid to the mean of its fit-set members rounded half up to
    uint8 -- this project's choice: the next assignment stays on the exact int8-MFMA path and the whole fit is reproducible -- an
    empty bin keeping its centroid.  The fit stops when an iteration's fit-set labels equal the previous one's (``converged``) or after
    ``max_iter`` iterations (rounded centroids do not guarantee a monotone objective); ``iterations`` counts the assignments, and
    after an unconverged fit the images are assigned once more, to the final centroids.  Three 1-element host reads per iteration (the
    comparison of the labels, the label check and the bincount of ``cluster.cluster_sums_u8``); a fit happens once per growth stage.
    UNPINNED, like the SWD and MS-SSIM: comparable between runs of this project, not with published tables.

    ``feed(samples_fp32)`` rounds to the 0..255 levels of the saved image (``ops.quantize_u8`` with ``drange``); ``feed_u8`` takes
    levels.  Batches of any size >= 1.  ``device``: None = where the source is; 'cpu' = the numpy twin in int64, equal bit for bit."""

    def __init__(self, source, k=50, holdout=0, seed=0, max_iter=30, z_threshold=Z_THRESHOLD_05, drange=(-1, 1), device=None):
        M, src_device = self._stack_source(source)
        from . import cluster
        if not 1 <= M <= cluster.MAX_IMAGES:
            raise ValueError('%d images (1 <= M <= %d: the per-bin sums are int32)' % (M, cluster.MAX_IMAGES))
        self.k = _int_in(k, 2, ops.NN_MAX_QUERIES, 'k = %r (2 <= k <= %d)' % (k, ops.NN_MAX_QUERIES))
        self.holdout = _int_in(holdout, 0, M - self.k, 'holdout = %r for %d images and k = %d (0 <= holdout < M - k + 1)' % (holdout, M, self.k))
        self.max_iter = _int_in(max_iter, 1, None, 'max_iter must be a positive integer, got %r' % (max_iter,))
        if not float(z_threshold) > 0:
            raise ValueError('z_threshold must be positive, got %r' % (z_threshold,))
        self.seed, self.z_threshold = int(seed), float(z_threshold)
        super(NDB, self).__init__(source, src_device, drange, device)
        self.num_images = M
        self.centroids = self.labels = self.ref = self.iterations = self.converged = self.resolution = self.shape = None
        self.reset()

    def split(self):
        """(held-out indices [h], fit-set indices [M - h]) as int64 CPU tensors: disjoint, together 0 .. M-1."""
        perm = torch.randperm(self.num_images, generator=torch.Generator().manual_seed(self.seed))
        return perm[:self.holdout], perm[self.holdout:]

    def fit(self):
        """Cluster the stack of the current stage; stores ``centroids`` uint8 [k,C,r,r] and ``labels`` int32 [M] (on ``device``), ``ref``
        (int64 [k], host), ``iterations``, ``converged``, ``resolution``; forgets what was fed.  Returns self."""
        stack = self.stack().contiguous()
        M, K = stack.shape[0], self.k
        if M != self.num_images:
            raise ValueError('the source holds %d images now, %d at construction' % (M, self.num_images))
        _, D = ops._image_bytes(stack, 'NDB.fit')
        held, fit = self.split()
        init = fit[torch.randperm(fit.numel(), generator=torch.Generator().manual_seed(self.seed + 1))[:K]]
        if self.device.type == 'cuda':
            from . import cluster
            is_fit = torch.zeros(M, dtype=torch.bool)
            is_fit[fit] = True
            is_fit = is_fit.to(self.device)
            outside = torch.full((M,), -1, dtype=torch.int32, device=self.device)
            c = stack.index_select(0, init.to(self.device)).contiguous()
            prev, iterations, converged = None, 0, False
            while iterations < self.max_iter:
                label, _ = cluster.assign_u8(stack, c)
                iterations += 1
                members = torch.where(is_fit, label, outside)
                if prev is not None and bool(torch.equal(members, prev)):
                    converged = True
                    break
                sums, counts = cluster.cluster_sums_u8(stack, members, K)
                c = cluster.centroids_u8(sums, counts, c)
                prev = members
            if not converged:
                label, _ = cluster.assign_u8(stack, c)
            counted = label.index_select(0, (held if self.holdout else fit).to(self.device)).to(torch.int64)
            ref = torch.bincount(counted, minlength=K).cpu().numpy().astype(np.int64)
            self.centroids, self.labels = c, label
        else:
            x = stack.numpy().reshape(M, D)
            is_fit = np.zeros(M, dtype=bool)
            is_fit[fit.numpy()] = True
            c = x[init.numpy()].copy()
            prev, iterations, converged = None, 0, False
            while iterations < self.max_iter:
                label, _ = _assign_host(x, c)
                iterations += 1
                members = np.where(is_fit, label, np.int32(-1)).astype(np.int32)
                if prev is not None and np.array_equal(members, prev):
                    converged = True
                    break
                c = _update_host(x, members, c)
                prev = members
            if not converged:
                label, _ = _assign_host(x, c)
            ref = np.bincount(label[(held if self.holdout else fit).numpy()], minlength=K).astype(np.int64)
            self.centroids, self.labels = torch.from_numpy(c.reshape((K,) + tuple(stack.shape[1:]))), torch.from_numpy(label)
        self.ref, self.iterations, self.converged = ref, iterations, converged
        self.shape, self.resolution = tuple(stack.shape[1:]), int(stack.shape[-1])
        self.reset()
        return self

    def reset(self):
        """Forget what was fed; the fit is kept."""
        self.gen = np.zeros(self.k, dtype=np.int64)
        self._counts = None                                             # device: the running histogram, read once in result()
        self._fed = 0
        self._result = None

    def _take(self, images):
        """Count a batch per bin."""
        n = images.shape[0]
        if self.device.type == 'cuda':
            from . import cluster
            images = images.contiguous()
            for a in range(0, n, ops.NN_MAX_QUERIES * 64):              # (any size: the distances of a chunk are [k, chunk] int64)
                label, _ = cluster.assign_u8(images[a:a + ops.NN_MAX_QUERIES * 64], self.centroids)
                counts = torch.bincount(label.to(torch.int64), minlength=self.k)
                self._counts = counts if self._counts is None else self._counts + counts
        else:
            label, _ = _assign_host(images.numpy().reshape(n, -1), self.centroids.numpy().reshape(self.k, -1))
            self.gen = self.gen + np.bincount(label, minlength=self.k).astype(np.int64)

    def result(self):
        """{'ndb', 'ndb_over_k', 'jsd', 'z' (float64 [k]), 'ref', 'gen' (int64 [k]), 'k', 'num_samples', 'iterations', 'converged'}
        in fp64 on the host (``ndb_statistic``).  One device synchronisation."""
        if self._result is None:
            if self.centroids is None:
                raise RuntimeError('fit() first')
            if self._fed < 1:
                raise RuntimeError('nothing was fed')
            if self._counts is not None:
                self.gen = self._counts.cpu().numpy().astype(np.int64)
            res = ndb_statistic(self.ref, self.gen, self.z_threshold)
            res.update(ref=self.ref.copy(), gen=self.gen.copy(), k=self.k, num_samples=self._fed, iterations=self.iterations,
                       converged=self.converged)
            self._result = res
        return self._result


# ------------------------------------------------------------------------- precision / recall / density / coverage (k-NN balls)
def _radii_host(x, k):
    """``ops.prd_kth_u8`` in numpy int64: x [N,D] uint8 -> int64 [N], the k-th smallest distance to an image at ANOTHER INDEX."""
    d = _d2_host(x, x)
    np.fill_diagonal(d, np.iinfo(np.int64).max)
    return np.partition(d, k - 1, axis=1)[:, k - 1].copy()


def _ball_host(a, b, rad_a=None, rad_b=None):
    """``ops.prd_ball_u8`` in numpy int64: (a_cnt, a_hit, b_cnt, b_hit) int32, None where the radius vector is."""
    d = _d2_host(a, b)
    a_cnt = b_hit = b_cnt = a_hit = None
    if rad_b is not None:
        inside = d <= np.asarray(rad_b, dtype=np.int64)[None]
        a_cnt, b_hit = inside.sum(axis=1).astype(np.int32), inside.sum(axis=0).astype(np.int32)
    if rad_a is not None:
        inside = d <= np.asarray(rad_a, dtype=np.int64)[:, None]
        b_cnt, a_hit = inside.sum(axis=0).astype(np.int32), inside.sum(axis=1).astype(np.int32)
    return a_cnt, a_hit, b_cnt, b_hit


def prd_statistic(fake_cnt, real_hit, real_cnt, k):
    """The four numbers from the counts of one pass with a = fakes and b = reals (``ops.prd_ball_u8``): ``fake_cnt[g]`` real balls
    fake g is inside, ``real_hit[r]`` fakes inside the ball of real r, ``real_cnt[r]`` fake balls real r is inside; integer counts, one
    fp64 division each."""
    fake_cnt, real_hit, real_cnt = (np.asarray(v, dtype=np.int64) for v in (fake_cnt, real_hit, real_cnt))
    ng, nr = fake_cnt.size, real_hit.size
    return {'precision': int((fake_cnt > 0).sum()) / float(ng), 'density': int(fake_cnt.sum()) / float(int(k) * ng),
            'coverage': int((real_hit > 0).sum()) / float(nr), 'recall': int((real_cnt > 0).sum()) / float(nr)}


class PrecisionRecall(_StackSource, _FittedFeed, _LevelMetric):
    """Improved precision and recall (Kynkaanniemi et al. 2019) with density and coverage (Naeem et al. 2020) in uint8 image space:
    fidelity and coverage as separate numbers on one scale.  Every image carries the ball whose radius is the distance to its ``k``-th
    nearest neighbour in its own set (``rad_k``: the k-th smallest exact squared L2 distance to an image at another index; a probe ON
    the boundary of a ball is inside).  With reals R and fakes G,

        precision = the fraction of fakes inside at least one real ball      density  = sum over fakes of #real balls it is in / (k |G|)
        recall    = the fraction of reals inside at least one fake ball      coverage = the fraction of reals whose ball holds a fake

    Defined per image vector: 1-, 2-, 3- and 4-channel networks are measured alike, and no feature network is involved.  Integer
    arithmetic: exact, the same bits from run to run, and ``device='cpu'`` (the numpy twin in int64) equals the device bit for bit.

    ``source``: a ``DeviceImageDataset`` or a ``DeviceStripDataset`` (``fit()`` takes ``level_stack()`` of the current ``model_depth``;
    ``range_in`` must be (0, 255)) or a uint8 tensor [M,C,r,r].  ``fit()`` keeps ``num_real`` images (None: all) -- the first entries of
    ``torch.randperm(M)`` from a CPU generator seeded ``seed`` -- reduced to ``max_resolution`` when the stage is finer (``ops.pyramid_
    level_u8``; None keeps the stage's resolution; the fakes are reduced alike), and their radii.  ``feed(samples_fp32)`` rounds to the
    0..255 levels of the saved image (``ops.quantize_u8`` with ``drange``); ``feed_u8`` takes levels; batches of any size >= 1, at the
    stage's resolution.  ``result()`` needs at least k + 1 fakes.  An evaluation is three tile passes (``ops.prd_kth_u8`` over the reals
    at ``fit()``, over the fakes, and one ``ops.prd_ball_u8`` with a = fakes, b = reals) and one host read.  D = C r^2 after the
    reduction must be a multiple of 16.  UNPINNED, like the SWD, MS-SSIM and NDB: comparable between runs of this project, not with
    published tables (those are over VGG features)."""

    def __init__(self, source, k=3, num_real=None, max_resolution=None, seed=0, drange=(-1, 1), device=None):
        _, src_device = self._stack_source(source)
        self.k = _int_in(k, 1, ops.NN_MAX_TOPK, 'k = %r (1 <= k <= %d)' % (k, ops.NN_MAX_TOPK))
        self.num_real = self.max_resolution = None
        if num_real is not None:
            self.num_real = _int_in(num_real, self.k + 1, None, 'num_real = %r for k = %d (at least k + 1 images)' % (num_real, self.k))
        if max_resolution is not None:
            message = 'max_resolution must be a power of two, got %r' % (max_resolution,)
            self.max_resolution = _int_in(max_resolution, 1, None, message)
            if self.max_resolution & (self.max_resolution - 1):
                raise ValueError(message)
        self.seed = int(seed)
        super(PrecisionRecall, self).__init__(source, src_device, drange, device)
        self.reals = self.radii = self.resolution = self.shape = self.indices = None
        self.reset()

    def _reduce(self, images):
        """uint8 [n,C,r,r] at the stage's resolution -> at min(r, max_resolution), on ``device``."""
        r = int(images.shape[-1])
        if self.max_resolution is None or r <= self.max_resolution:
            return images.contiguous()
        depthdiff = (r // self.max_resolution).bit_length() - 1
        if self.device.type == 'cuda':
            return ops.pyramid_level_u8(images.contiguous(), depthdiff)
        from .dataset import level_host
        return torch.from_numpy(np.ascontiguousarray(level_host(images.numpy(), depthdiff)))

    def fit(self):
        """Take the reals of the current stage and their radii; stores ``reals`` uint8 [num_real,C,r',r'] and ``radii`` int64
        [num_real] (on ``device``), ``indices`` (int64, host: the images taken), ``resolution`` (the STAGE's, what ``feed`` expects);
        forgets what was fed.  Returns self."""
        stack = self.stack()
        M = stack.shape[0]
        n = M if self.num_real is None else self.num_real
        if not self.k + 1 <= n <= M:
            raise ValueError('%d of %d images for k = %d (k + 1 <= num_real <= M)' % (n, M, self.k))
        self.indices = torch.randperm(M, generator=torch.Generator().manual_seed(self.seed))[:n]
        reals = self._reduce(stack.index_select(0, self.indices.to(self.device)))
        ops._image_bytes(reals, 'PrecisionRecall.fit')
        if self.device.type == 'cuda':
            self.radii = ops.prd_kth_u8(reals, self.k)
        else:
            self.radii = torch.from_numpy(_radii_host(reals.numpy().reshape(n, -1), self.k))
        self.reals, self.shape, self.resolution = reals, tuple(stack.shape[1:]), int(stack.shape[-1])
        self.reset()
        return self

    def reset(self):
        """Forget what was fed; the fit is kept."""
        self._fakes, self._fed, self._result = [], 0, None

    def _take(self, images):
        """Keep a batch, reduced like the reals."""
        self._fakes.append(self._reduce(images))

    def result(self):
        """{'precision', 'recall', 'density', 'coverage' (fp64), 'num_real', 'num_fake', 'k'}.  One device synchronisation."""
        if self._result is None:
            if self.reals is None:
                raise RuntimeError('fit() first')
            if self._fed < self.k + 1:
                raise RuntimeError('%d images were fed; the radii of the fakes need k + 1 = %d' % (self._fed, self.k + 1))
            fakes = self._fakes[0] if len(self._fakes) == 1 else torch.cat(self._fakes)
            if self.device.type == 'cuda':
                fakes = fakes.contiguous()
                fake_cnt, _, real_cnt, real_hit = ops.prd_ball_u8(fakes, self.reals, ops.prd_kth_u8(fakes, self.k), self.radii)
                counts = torch.cat([fake_cnt, real_hit, real_cnt]).cpu().numpy()
            else:
                f, r = fakes.numpy().reshape(self._fed, -1), self.reals.numpy().reshape(self.reals.shape[0], -1)
                fake_cnt, _, real_cnt, real_hit = _ball_host(f, r, _radii_host(f, self.k), self.radii.numpy())
                counts = np.concatenate([fake_cnt, real_hit, real_cnt])
            nr = self.reals.shape[0]
            res = prd_statistic(counts[:self._fed], counts[self._fed:self._fed + nr], counts[self._fed + nr:], self.k)
            res.update(num_real=nr, num_fake=self._fed, k=self.k)
            self._result = res
        return self._result


# ------------------------------------------------------------------------- Frechet distance over a random convolutional embedding
EMBED_FEATURES = 128                # features of an embedded image: the width of the 4x4 layer
EMBED_SLOPE, EMBED_EPS = 0.2, 1e-8
EMBED_MAX_RESOLUTION = 512          # embed_width(1024) = 4 is no multiple of 8: pg_smp_conv3_bf16 does not take it


def embed_width(H):
    """Output channels of the embedding's 3x3 layer at map size ``H``."""
    return min(EMBED_FEATURES, 4096 // H)


def _pow2_at_least_4(v, message):
    v = _int_in(v, 4, None, message)
    if v & (v - 1):
        raise ValueError(message)
    return v


def _rne_bf16_host(t):
    """Round an fp64 tensor of finite values to nearest even onto the bf16 grid (subnormals included); fp64 out."""
    _, e = torch.frexp(t)
    u = torch.ldexp(torch.ones_like(t), e.clamp(min=-125) - 8)
    return torch.round(t / u) * u


def _moments_host(x):
    """``ops.fd_moments_f64`` in numpy float64: (mean [F], cov [F,F]), cov mirrored from its upper triangle."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.sum(axis=0) / x.shape[0]
    a = x - mean
    cov = np.triu(a.T.dot(a) / (x.shape[0] - 1))
    return mean, cov + np.triu(cov, 1).T


class RandomEmbedding(object):
    """A randomly initialised convolutional embedding of uint8 images (Naeem et al. 2020 propose one for data far from ImageNet):
    ``embedding(images_u8 [n,C,r,r]) -> features [n,128]`` in fp32, on ``device``.  r a power of two >= 4; above ``max_resolution`` the
    images are first reduced with ``ops.pyramid_level_u8``.  1 <= C <= 4.

    The network: the stem ``rne_bf16((x - 127.5) / 127.5)`` into 8 NHWC channels (zeros above C; ``ops.emb_stem_u8_bf16``); then for
    H = r, r/2, ..., 4 one 3x3 pad-1 layer of ``embed_width(H) = min(128, 4096 // H)`` output channels on the bf16 matrix cores
    (``sampling.conv3_bf16``: no bias, leaky ReLU 0.2, fused PixelNorm with eps 1e-8, scale sqrt(2 / (9 Cin)), ONE rounding to bf16),
    followed while H > 4 by the 2x2 mean ``ops.emb_pool2_bf16``; the 4x4 map is averaged in fp32 (``ops.emb_gap_f32``).  The layer at
    map size H with Cin input channels has the weights ``torch.randn(Cout, Cin, 3, 3)`` of a CPU generator seeded
    ``seed * 1000003 + H``, permuted to [3,3,Cout,Cin] and rounded to bf16 once; they are uploaded once and kept.  A layer below the
    first therefore has the same weights whatever r is, and the same seed gives the same embedding on every machine; the first layer
    (Cin = 8, the padded stem) is a draw of its own from the same seed.  ``max_resolution`` <= 512: at 1024 the rule gives 4 output
    channels, which the conv kernel does not take.

    Images are embedded ``chunk`` at a time, which bounds the activations (64 images of 256^2 x 16 channels are 128 MiB in bf16).  Every
    stage has one writer per element and a fixed order: two calls give the same bits, whatever ``chunk`` is.

    ``device='cpu'`` evaluates the same contract on the host -- torch CPU convolutions in float64 over the bf16-rounded operands with
    the same rounding points; stem, pool and mean exactly as the kernels -- which is CLOSE to the device, not equal: a conv output
    within a rounding error of a bf16 tie may round the other way."""

    def __init__(self, channels, seed=0, max_resolution=256, chunk=64, device=None):
        self.channels = _int_in(channels, 1, ops.EMB_MAX_C, 'channels = %r (1 <= channels <= %d)' % (channels, ops.EMB_MAX_C))
        self.seed = _int_in(seed, None, None, 'seed = %r (an integer)' % (seed,))
        message = 'max_resolution = %r (a power of two, 4 <= max_resolution <= %d)' % (max_resolution, EMBED_MAX_RESOLUTION)
        self.max_resolution = _pow2_at_least_4(max_resolution, message)
        if self.max_resolution > EMBED_MAX_RESOLUTION:
            raise ValueError(message)
        self.chunk = _int_in(chunk, 1, None, 'chunk = %r (at least 1)' % (chunk,))
        self.device = torch.device('cuda' if device is None else device)
        self._weights = {}

    def layers(self, r):
        """[(H, Cin, Cout)] of the 3x3 layers for images of (reduced) resolution ``r``."""
        out, cin = [], ops.EMB_STEM_CH
        while r >= 4:
            out.append((r, cin, embed_width(r)))
            cin, r = embed_width(r), r // 2
        return out

    def weights(self, H, cin):
        """bf16 [3,3,Cout,Cin] of the layer at map size ``H`` with ``cin`` inputs, on ``device``."""
        key = (H, cin)
        if key not in self._weights:
            g = torch.Generator().manual_seed(self.seed * 1000003 + H)
            w = torch.randn(embed_width(H), cin, 3, 3, generator=g)
            self._weights[key] = w.permute(2, 3, 0, 1).contiguous().to(torch.bfloat16).to(self.device)
        return self._weights[key]

    def _check(self, images):
        if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[0] < 1 \
                or images.shape[1] != self.channels or images.shape[2] != images.shape[3]:
            raise ValueError('expected uint8 images [n,%d,r,r], got %s'
                             % (self.channels, tuple(images.shape) if torch.is_tensor(images) else type(images)))
        _pow2_at_least_4(int(images.shape[-1]), 'images of %d x %d (r a power of two >= 4)' % tuple(images.shape[2:]))

    def _reduce(self, images):
        r = int(images.shape[-1])
        if r <= self.max_resolution:
            return images.contiguous()
        depthdiff = (r // self.max_resolution).bit_length() - 1
        if self.device.type == 'cuda':
            return ops.pyramid_level_u8(images.contiguous(), depthdiff)
        from .dataset import level_host
        return torch.from_numpy(np.ascontiguousarray(level_host(images.numpy(), depthdiff)))

    def _device_chunk(self, images, trace):
        from . import sampling
        n, r = images.shape[0], int(images.shape[-1])
        x = ops.emb_stem_u8_bf16(images)
        trace.append(('stem', x))
        for H, cin, _ in self.layers(r):
            x = sampling.conv3_bf16(x, self.weights(H, cin), None, n, H, H, math.sqrt(2.0 / (9 * cin)), EMBED_SLOPE, EMBED_EPS,
                                    pixelnorm=True)
            trace.append(('conv%d' % H, x))
            if H > 4:
                x = ops.emb_pool2_bf16(x)
                trace.append(('pool%d' % H, x))
        f = ops.emb_gap_f32(x)
        trace.append(('gap', f))
        return f

    def _host_chunk(self, images, trace):
        import torch.nn.functional as F
        r, C = int(images.shape[-1]), self.channels
        x32 = (images.to(torch.float32) - 127.5) / 127.5                    # float32: one rounding per operation, as the stem kernel
        x = x32.to(torch.bfloat16).double()                                 # NCHW; the stem's zero channels contribute nothing
        trace.append(('stem', x))
        for H, cin, _ in self.layers(r):
            w = self.weights(H, cin).double().permute(2, 3, 0, 1)[:, :x.shape[1]]
            v = math.sqrt(2.0 / (9 * cin)) * F.conv2d(x, w, None, 1, 1)
            v = torch.where(v > 0, v, v * EMBED_SLOPE)
            x = _rne_bf16_host(v / torch.sqrt(torch.mean(v * v, 1, keepdim=True) + EMBED_EPS))
            trace.append(('conv%d' % H, x))
            if H > 4:
                a = x.float()                                               # bf16 values: exact in float32
                p = ((a[:, :, 0::2, 0::2] + a[:, :, 0::2, 1::2]) + (a[:, :, 1::2, 0::2] + a[:, :, 1::2, 1::2])) * 0.25
                x = p.to(torch.bfloat16).double()
                trace.append(('pool%d' % H, x))
        a = x.float()
        s = torch.zeros(a.shape[:2], dtype=torch.float32)
        for h in range(a.shape[2]):
            for w_ in range(a.shape[3]):
                s = s + a[:, :, h, w_]
        f = s * (torch.ones((), dtype=torch.float32) / float(a.shape[2] * a.shape[3]))
        trace.append(('gap', f))
        return f

    def trace(self, images):
        """[(name, tensor)] of every stage's output for ONE chunk of images: 'stem', then 'conv<H>' and 'pool<H>' per layer, 'gap'.
        Device mode: bf16 NHWC maps; host mode: fp64 NCHW maps of bf16 values (the stem without its zero channels)."""
        self._check(images)
        out = []
        images = self._reduce(images.to(self.device))
        (self._device_chunk if self.device.type == 'cuda' else self._host_chunk)(images, out)
        return out

    def __call__(self, images):
        self._check(images)
        images = images.to(self.device)
        run = self._device_chunk if self.device.type == 'cuda' else self._host_chunk
        out = [run(self._reduce(images[s:s + self.chunk]), []) for s in range(0, images.shape[0], self.chunk)]
        return out[0] if len(out) == 1 else torch.cat(out)


def frechet_statistic(mu1, cov1, mu2, cov2):
    """The Frechet distance between two Gaussians from their moments, in fp64 on the host:

        fd = |mu1 - mu2|^2 + tr cov1 + tr cov2 - 2 sum_k sqrt(max(lambda_k, 0))

    with lambda the eigenvalues of S cov2 S and S = cov1^(1/2) from a symmetric eigendecomposition whose negative eigenvalues are
    clamped to 0 -- S cov2 S is symmetric and has the eigenvalues of cov1 cov2, so only ``eigh`` / ``eigvalsh`` are needed and no general
    matrix square root.  Returns {'fd', 'mean_term', 'cov_term'}: fd = mean_term + cov_term, as computed -- NOT clamped at 0 (equal
    moments give a value within rounding of 0, of either sign)."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64), np.asarray(mu2, dtype=np.float64)
    cov1, cov2 = np.asarray(cov1, dtype=np.float64), np.asarray(cov2, dtype=np.float64)
    F = mu1.size
    if mu1.shape != (F,) or mu2.shape != (F,) or cov1.shape != (F, F) or cov2.shape != (F, F):
        raise ValueError('frechet_statistic: mu [F] and cov [F,F] of both sets, got %s, %s, %s, %s' % (mu1.shape, cov1.shape, mu2.shape, cov2.shape))
    lam, V = np.linalg.eigh(cov1)
    S = (V * np.sqrt(np.maximum(lam, 0.0))).dot(V.T)
    A = S.dot(cov2).dot(S)
    lam = np.linalg.eigvalsh(0.5 * (A + A.T))
    mean_term = float(((mu1 - mu2) ** 2).sum())
    cov_term = float(np.trace(cov1) + np.trace(cov2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())
    return {'fd': mean_term + cov_term, 'mean_term': mean_term, 'cov_term': cov_term}


class FrechetDistance(_StackSource, _FittedFeed, _LevelMetric):
    """The Frechet distance ``fd`` between the training images and generated images over the features of a ``RandomEmbedding``: the
    distance between the Gaussians with the two sets' feature means and covariances.  It is NOT the Inception distance: no pretrained
    network is involved (none can be shipped, and ImageNet features would be the wrong ones for one- and two-channel spectrograms), so
    the value is UNPINNED like the SWD, MS-SSIM, NDB and PRD -- comparable between runs of this project with the same seed and
    ``max_resolution``, not with published FID tables.  1- to 4-channel networks are measured alike.

    ``source``: a ``DeviceImageDataset`` or a ``DeviceStripDataset`` (``fit()`` takes ``level_stack()`` of the current ``model_depth``;
    ``range_in`` must be (0, 255)) or a uint8 tensor [M,C,r,r].  ``fit()`` embeds ``num_real`` images (None: all) -- the first entries of
    ``torch.randperm(M)`` from a CPU generator seeded ``seed`` -- and keeps their mean and covariance (``ops.fd_moments_f64``: fp64, on
    the fp64 matrix cores, reproducible).  ``feed(samples_fp32)`` rounds to the 0..255 levels of the saved image (``ops.quantize_u8``
    with ``drange``); ``feed_u8`` takes levels; batches of any size >= 1, at the stage's resolution; their [n,128] features are kept.
    ``result()`` needs at least 2 fed images: one moments call over all fed features, one host read, ``frechet_statistic`` in fp64 on
    the host.  ``embedding``: a ``RandomEmbedding`` to use (and share between metrics) instead of one made from ``seed`` and
    ``max_resolution`` at ``fit()``.  ``device='cpu'``: the host twin (the embedding's host mode and numpy moments), close to the device
    but not equal.

    With fewer samples than the 128 features on either side a covariance estimate is rank deficient: the value is finite and still
    ordered sensibly, but biased; use thousands of images per set, and compare values taken with the same counts."""

    def __init__(self, source, num_real=None, max_resolution=256, seed=0, drange=(-1, 1), device=None, embedding=None):
        _, src_device = self._stack_source(source)
        self.num_real = None if num_real is None else _int_in(num_real, 2, None, 'num_real = %r (at least 2 images)' % (num_real,))
        self.seed = _int_in(seed, None, None, 'seed = %r (an integer)' % (seed,))
        super(FrechetDistance, self).__init__(source, src_device, drange, device)
        if embedding is None:
            RandomEmbedding(1, self.seed, max_resolution, device=self.device)     # (the argument check; made for C channels at fit())
        elif not isinstance(embedding, RandomEmbedding) or embedding.device.type != self.device.type:
            raise ValueError('embedding: expected a RandomEmbedding on %s' % self.device.type)
        self.max_resolution, self.embedding = max_resolution, embedding
        self.mean = self.cov = self.resolution = self.shape = self.indices = None
        self.reset()

    def _moments(self, feats):
        if self.device.type == 'cuda':
            return ops.fd_moments_f64(feats.contiguous())
        return tuple(torch.from_numpy(v) for v in _moments_host(feats.numpy()))

    def fit(self, block=1024):
        """Embed the reals of the current stage, ``block`` at a time, and keep their moments: ``mean`` [128] and ``cov`` [128,128] (fp64,
        on ``device``), ``indices`` (int64, host: the images taken), ``resolution`` (the STAGE's, what ``feed`` expects); forgets what was
        fed.  Returns self."""
        stack = self.stack()
        M, C = stack.shape[0], stack.shape[1]
        n = M if self.num_real is None else self.num_real
        if not 2 <= n <= M:
            raise ValueError('%d of %d images (2 <= num_real <= M)' % (n, M))
        if self.embedding is None:
            self.embedding = RandomEmbedding(C, self.seed, self.max_resolution, device=self.device)
        if self.embedding.channels != C:
            raise ValueError('the embedding takes %d channels, the stack has %d' % (self.embedding.channels, C))
        self.indices = torch.randperm(M, generator=torch.Generator().manual_seed(self.seed))[:n]
        idx = self.indices.to(self.device)
        feats = [self.embedding(stack.index_select(0, idx[s:s + block])) for s in range(0, n, block)]
        self.mean, self.cov = self._moments(feats[0] if len(feats) == 1 else torch.cat(feats))
        self.shape, self.resolution = tuple(stack.shape[1:]), int(stack.shape[-1])
        self.reset()
        return self

    def reset(self):
        """Forget what was fed; the fit is kept."""
        self._feats, self._fed, self._result = [], 0, None

    def _take(self, images):
        self._feats.append(self.embedding(images))

    def result(self):
        """{'fd', 'mean_term', 'cov_term' (fp64), 'num_real', 'num_fake'}.  One device synchronisation."""
        if self._result is None:
            if self.mean is None:
                raise RuntimeError('fit() first')
            if self._fed < 2:
                raise RuntimeError('%d images were fed; a covariance needs 2' % self._fed)
            mean, cov = self._moments(self._feats[0] if len(self._feats) == 1 else torch.cat(self._feats))
            F = mean.numel()
            host = torch.cat([self.mean, self.cov.reshape(-1), mean, cov.reshape(-1)]).cpu().numpy()
            mu1, cov1, mu2, cov2 = host[:F], host[F:F + F * F], host[F + F * F:2 * F + F * F], host[2 * F + F * F:]
            res = frechet_statistic(mu1, cov1.reshape(F, F), mu2, cov2.reshape(F, F))
            res.update(num_real=int(self.indices.numel()), num_fake=self._fed)
            self._result = res
        return self._result


# ------------------------------------------------------------------------- kernel distance: unbiased MMD^2 over the same embedding
KID_SUBSET = 1024                   # rows of one subset of ``kid_statistic``: the default of Binkowski et al. is 1000; a multiple of the tile


def _kid_tilesums_host(x, y=None, gamma=None, coef0=1.0, skip_diagonal=False):
    """``ops.kid_tilesums_f64`` in numpy float64: [A,B] sums of ``(gamma x_i . y_j + coef0)^3`` per 64 x 64 tile, the kernel function
    applied before the pairs of a ragged tile (and i == j under ``skip_diagonal``) are left out.  1024 rows at a time: the Gram matrix
    of 30 000 reals never exists here either.  The order of the sums is numpy's, not the device's."""
    T = ops.KID_TILE
    x = np.asarray(x, dtype=np.float64)
    self_form = y is None
    y = x if self_form else np.asarray(y, dtype=np.float64)
    if skip_diagonal and not self_form:
        raise ValueError('skip_diagonal is for the self form (y = None)')
    (M, F), N = x.shape, y.shape[0]
    gamma = 1.0 / F if gamma is None else float(gamma)
    A, B = (M + T - 1) // T, (N + T - 1) // T
    out = np.zeros((A, B), dtype=np.float64)
    for r0 in range(0, M, 16 * T):
        t = gamma * x[r0:r0 + 16 * T].dot(y.T) + float(coef0)
        k = (t * t) * t
        if skip_diagonal:
            i = np.arange(r0, r0 + k.shape[0])
            k[i - r0, i] = 0.0
        rows = (k.shape[0] + T - 1) // T
        padded = np.zeros((rows * T, B * T), dtype=np.float64)
        padded[:k.shape[0], :N] = k
        out[r0 // T:r0 // T + rows] = padded.reshape(rows, T, B, T).sum(axis=(1, 3))
    return out


def kid_statistic(sxx, syy, sxy, m, n, subset_size=None):
    """The unbiased estimator of the squared maximum mean discrepancy (the Kernel Inception Distance estimator of Binkowski et al.
    2018) from the tile sums of the kernel (``ops.kid_tilesums_f64``), in fp64 on the host:

        kid = sum(sxx) / (m (m - 1)) + sum(syy) / (n (n - 1)) - 2 sum(sxy) / (m n)

    ``sxx`` [A,A] and ``syy`` [B,B]: the self forms of the two sets of ``m`` and ``n`` vectors taken with ``skip_diagonal``; ``sxy``
    [A,B]: the cross form.  Unbiased at any sample count and NOT clamped at 0: two sets from one distribution give values of either
    sign around 0.  ``subset_size`` (None: ``KID_SUBSET`` = 1024; a multiple of ``ops.KID_TILE``): the same estimator on each of the
    ``min(m, n) // subset_size`` subsets, subset s being rows [s subset_size, (s + 1) subset_size) of BOTH sets -- read out of the same
    tile sums, whose tiles are whole there.  Returns {'kid', 'subsets' (their number), 'kid_subset_mean', 'kid_subset_std' (the sample
    standard deviation, n - 1 in the denominator)}; the last two are None with fewer than 2 subsets."""
    T = ops.KID_TILE
    m = _int_in(m, 2, None, 'm = %r (at least 2 vectors a set)' % (m,))
    n = _int_in(n, 2, None, 'n = %r (at least 2 vectors a set)' % (n,))
    S = KID_SUBSET if subset_size is None else _int_in(subset_size, T, None, 'subset_size = %r (a positive multiple of %d)' % (subset_size, T))
    if S % T:
        raise ValueError('subset_size = %r (a positive multiple of %d)' % (subset_size, T))
    sxx, syy, sxy = (np.asarray(s, dtype=np.float64) for s in (sxx, syy, sxy))
    A, B = (m + T - 1) // T, (n + T - 1) // T
    if sxx.shape != (A, A) or syy.shape != (B, B) or sxy.shape != (A, B):
        raise ValueError('kid_statistic: tile sums %s, %s, %s for m = %d, n = %d (expected %s, %s, %s)'
                         % (sxx.shape, syy.shape, sxy.shape, m, n, (A, A), (B, B), (A, B)))
    kid = float(sxx.sum() / (m * (m - 1.0)) + syy.sum() / (n * (n - 1.0)) - 2.0 * sxy.sum() / (float(m) * n))
    t = S // T
    values = []
    for s in range(min(m, n) // S):
        b = slice(s * t, (s + 1) * t)
        values.append(float(sxx[b, b].sum() / (S * (S - 1.0)) + syy[b, b].sum() / (S * (S - 1.0)) - 2.0 * sxy[b, b].sum() / (float(S) * S)))
    many = len(values) >= 2
    return {'kid': kid, 'subsets': len(values), 'kid_subset_mean': float(np.mean(values)) if many else None,
            'kid_subset_std': float(np.std(values, ddof=1)) if many else None}


class KernelDistance(_StackSource, _FittedFeed, _LevelMetric):
    """The kernel distance ``kid`` between the training images and generated images over the features of a ``RandomEmbedding``: the
    unbiased estimator of the squared maximum mean discrepancy with the cubic polynomial kernel ``k(a, b) = (gamma a . b + coef0)^3``
    (the Kernel Inception Distance estimator of Binkowski et al. 2018; ``gamma`` None = 1 / 128, ``coef0`` = 1), ``kid_statistic``.
    Unlike ``fd`` it is unbiased at ANY sample count -- a few dozen images a side give a noisy value around the true one, not a value
    off by a hundred -- and it comes with a spread over subsets: the number to compare between runs on a small data set.  It is NOT
    the Inception-feature KID: no pretrained network is involved, so the value is UNPINNED like the other metrics -- comparable between
    runs of this project with the same seed and ``max_resolution``, not with published tables.  It is not clamped at 0.

    ``source``, ``num_real``, ``max_resolution``, ``seed``, ``drange``, ``embedding`` and the ``fit / reset / feed / feed_u8 / result``
    protocol are ``FrechetDistance``'s, the same ``torch.randperm(M)`` choice of reals included.  ``fit()`` keeps the reals' features
    ``features`` [n,128] fp32 (15 MB for 30 000) and their tile sums ``sxx`` (``ops.kid_tilesums_f64``, self form, ``skip_diagonal``: fp64
    on the fp64 matrix cores, reproducible; no Gram matrix is written).  ``result()`` needs at least 2 fed images: one self call over the fed
    features (``syy``), one cross call (``sxy``), one host read, ``kid_statistic`` with ``subset_size`` in fp64 on the host.
    ``with_fd``: also the Frechet distance of the same features (``ops.fd_moments_f64``, ``frechet_statistic``), exactly the ``fd`` of a
    ``FrechetDistance`` with the same seed, embedding and feeds -- one set of generator passes and one embedding serve both numbers.
    ``device='cpu'``: the host twin (the embedding's host mode, ``_kid_tilesums_host``), close to the device but not equal: the order
    of the sums differs."""

    def __init__(self, source, num_real=None, max_resolution=256, seed=0, drange=(-1, 1), device=None, embedding=None, subset_size=1024,
                 gamma=None, coef0=1.0, with_fd=False):
        _, src_device = self._stack_source(source)
        self.num_real = None if num_real is None else _int_in(num_real, 2, None, 'num_real = %r (at least 2 images)' % (num_real,))
        self.seed = _int_in(seed, None, None, 'seed = %r (an integer)' % (seed,))
        message = 'subset_size = %r (a positive multiple of %d)' % (subset_size, ops.KID_TILE)
        self.subset_size = KID_SUBSET if subset_size is None else _int_in(subset_size, ops.KID_TILE, None, message)
        if self.subset_size % ops.KID_TILE:
            raise ValueError(message)
        self.gamma, self.coef0, self.with_fd = None if gamma is None else float(gamma), float(coef0), bool(with_fd)
        super(KernelDistance, self).__init__(source, src_device, drange, device)
        if embedding is None:
            RandomEmbedding(1, self.seed, max_resolution, device=self.device)     # (the argument check; made for C channels at fit())
        elif not isinstance(embedding, RandomEmbedding) or embedding.device.type != self.device.type:
            raise ValueError('embedding: expected a RandomEmbedding on %s' % self.device.type)
        self.max_resolution, self.embedding = max_resolution, embedding
        self.features = self.sxx = self.syy = self.sxy = self.mean = self.cov = self.resolution = self.shape = self.indices = None
        self.reset()

    def _tilesums(self, x, y=None, skip_diagonal=False):
        if self.device.type == 'cuda':
            return ops.kid_tilesums_f64(x, y, self.gamma, self.coef0, skip_diagonal)
        return torch.from_numpy(_kid_tilesums_host(x.numpy(), None if y is None else y.numpy(), self.gamma, self.coef0, skip_diagonal))

    def _moments(self, feats):
        if self.device.type == 'cuda':
            return ops.fd_moments_f64(feats)
        return tuple(torch.from_numpy(v) for v in _moments_host(feats.numpy()))

    def fit(self, block=1024):
        """Embed the reals of the current stage, ``block`` at a time, and keep ``features`` [n,128] (fp32) and ``sxx`` (fp64 tile sums
        without the diagonal) on ``device`` -- with ``with_fd`` also ``mean`` and ``cov`` -- ``indices`` (int64, host: the images taken)
        and ``resolution`` (the STAGE's, what ``feed`` expects); forgets what was fed.  Returns self."""
        stack = self.stack()
        M, C = stack.shape[0], stack.shape[1]
        n = M if self.num_real is None else self.num_real
        if not 2 <= n <= M:
            raise ValueError('%d of %d images (2 <= num_real <= M)' % (n, M))
        if self.embedding is None:
            self.embedding = RandomEmbedding(C, self.seed, self.max_resolution, device=self.device)
        if self.embedding.channels != C:
            raise ValueError('the embedding takes %d channels, the stack has %d' % (self.embedding.channels, C))
        self.indices = torch.randperm(M, generator=torch.Generator().manual_seed(self.seed))[:n]
        idx = self.indices.to(self.device)
        feats = [self.embedding(stack.index_select(0, idx[s:s + block])) for s in range(0, n, block)]
        self.features = (feats[0] if len(feats) == 1 else torch.cat(feats)).contiguous()
        self.sxx = self._tilesums(self.features, skip_diagonal=True)
        self.mean, self.cov = self._moments(self.features) if self.with_fd else (None, None)
        self.shape, self.resolution = tuple(stack.shape[1:]), int(stack.shape[-1])
        self.reset()
        return self

    def reset(self):
        """Forget what was fed; the fit is kept."""
        self._feats, self._fed, self._result = [], 0, None
        self.syy = self.sxy = None

    def _take(self, images):
        self._feats.append(self.embedding(images))

    def result(self):
        """{'kid', 'subsets', 'kid_subset_mean', 'kid_subset_std' (fp64; ``kid_statistic``), 'num_real', 'num_fake'} and with ``with_fd``
        'fd', 'mean_term', 'cov_term'.  Leaves the tile sums of this evaluation in ``syy`` and ``sxy``.  One device synchronisation."""
        if self._result is None:
            if self.features is None:
                raise RuntimeError('fit() first')
            if self._fed < 2:
                raise RuntimeError('%d images were fed; the estimator needs 2' % self._fed)
            fake = (self._feats[0] if len(self._feats) == 1 else torch.cat(self._feats)).contiguous()
            self.syy = self._tilesums(fake, skip_diagonal=True)
            self.sxy = self._tilesums(self.features, fake)
            parts = [self.sxx, self.syy, self.sxy]
            if self.with_fd:
                parts += [self.mean, self.cov] + list(self._moments(fake))
            host = torch.cat([p.reshape(-1) for p in parts]).cpu().numpy()
            split = np.split(host, np.cumsum([p.numel() for p in parts])[:-1])
            m, n = int(self.indices.numel()), self._fed
            res = kid_statistic(split[0].reshape(self.sxx.shape), split[1].reshape(self.syy.shape), split[2].reshape(self.sxy.shape), m, n,
                                self.subset_size)
            if self.with_fd:
                F = split[3].size
                res.update(frechet_statistic(split[3], split[4].reshape(F, F), split[5], split[6].reshape(F, F)))
            res.update(num_real=m, num_fake=n)
            self._result = res
        return self._result
