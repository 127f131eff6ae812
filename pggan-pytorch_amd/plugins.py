"""Trainer plugins of the hot path: DepthManager and LRScheduler (/root/reference/plugins.py:13-99).

``torch.utils.trainer.plugins`` — the base classes the reference imports (plugins.py:8-9) — was removed
from PyTorch after 0.3, so the minimal ``Plugin`` protocol is restated here: an object with
``trigger_interval = [(n, unit), ...]``, ``register(trainer)`` and one method per unit
(``iteration`` / ``epoch`` / ``s`` / ``end``) — exactly what ``Trainer.call_plugins`` relies on.
All schedule arithmetic is Python int (+ one IEEE double division for alpha): bit-exact by construction."""
import math
import os
import time
import warnings
from datetime import timedelta
from glob import glob

from . import metrics
from .metrics import _int_in


class Plugin(object):
    """The plugin protocol ``Trainer`` dispatches on: ``trigger_interval`` = list of (period, unit) pairs, ``register(trainer)``,
    and one method per unit it listens on."""

    def __init__(self, interval=None):
        self.trigger_interval = [] if interval is None else interval

    def register(self, trainer):
        raise NotImplementedError


def _stat(stats, name, value, fmt='{val:.2f}', **extra):
    """One entry of ``trainer.stats`` under the convention the reference's ``Logger`` prints (``log_name``, ``log_epoch_fields``, ``val``)."""
    stats[name] = dict(log_name=name, log_epoch_fields=[fmt], val=value, **extra)


def _is_replica(trainer):
    """Replicas of a data-parallel run are identical: rank 0 alone writes and evaluates."""
    dp = getattr(trainer, 'parallel', None)
    return dp is not None and dp.rank != 0


def _check_smoothed(trainer, smoothed, who):
    if smoothed and getattr(trainer, 'g_ema', None) is None:
        raise ValueError('%s(smoothed=True) needs Trainer(g_ema=GeneratorEMA(G))' % who)


def _check_precision(precision, who):
    from .sampling import check_precision
    return check_precision(precision, '%s(precision=...)' % who)


def _output_generator(trainer, smoothed, precision='fp32'):
    """The network an output plugin evaluates: the smoothed generator Gs when the trainer keeps one (``smoothed=None``: use it if it is
    there; ``False``: raw G), at G's growth stage and ordered behind its last update.  ``precision='bf16'``: that network's
    ``sampling.Sampler`` instead -- the same ``forward(z)``, evaluated forward-only on the bf16 matrix cores (sampling.py has the
    contract).  Measured on an MI355X with 16 untrained images per call (docs/experiments_sampling.md): the bf16 pass is SLOWER than
    the fp32 one at the 1024x1024 stage (2.90 against 2.44 ms: 0.84x), ties it at 128x128 .. 512x512 (0.98 - 1.05x) and is slower below;
    the images differ by 1 % relative L2 and MS-SSIM / SWD at 256x256 move by less than a tenth of the metrics' own noise.  Until the
    bf16 kernels are tuned the keyword buys half-width activations, not time: every period default stays derived for 'fp32'."""
    from .sampling import generator_for
    _check_precision(precision, '_output_generator')
    ema = getattr(trainer, 'g_ema', None)
    return generator_for(trainer.G if ema is None or smoothed is False else ema.network(), precision)


def growth_stage(cur_nimg, lod_training_nimg, lod_transition_nimg, max_depth):
    """The progressive-growing schedule as a pure integer function of the images shown so far (behaviour of reference
    plugins.py:58-63, bit for bit): time is cut into cycles of ``stabilise`` (lod_training_nimg) + ``fade``
    (lod_transition_nimg) images; the stage index is the number of completed cycles plus the number of whole
    ``stabilise`` spans already inside the current one, clamped to ``max_depth``; while a new stage is still un-clamped
    and past its stabilise span, alpha is the position inside the remaining span over ``fade`` (one IEEE double division),
    otherwise exactly 1.0.  Returns (depth, alpha)."""
    cycle, inside = divmod(cur_nimg, lod_training_nimg + lod_transition_nimg)
    spans, position = divmod(inside, lod_training_nimg)
    stage = cycle + spans
    depth = stage if stage < max_depth else max_depth
    fading = spans > 0 and stage == depth
    return depth, (position / lod_transition_nimg if fading else 1.0)


class DepthManager(Plugin):
    """Growth-stage controller (reference plugins.py:13-81: same constructor arguments, same trainer/dataset fields
    written, same ``stats`` keys).  On a stage change it rebuilds the data iterator and the latent generator for the
    stage's minibatch size and sets the tick length; alpha is pushed to D, G and the dataset whenever it changes."""

    def __init__(self, create_dataloader_fun, create_rlg, max_depth, minibatch_default=16,
                 minibatch_overrides={6: 14, 7: 6, 8: 3}, tick_kimg_default=20,
                 tick_kimg_overrides={3: 10, 4: 10, 5: 5, 6: 2, 7: 2, 8: 1},
                 lod_training_nimg=100 * 1000, lod_transition_nimg=100 * 1000, max_lod=None, depth_offset=None):
        super(DepthManager, self).__init__([(1, 'iteration')])
        self.create_dataloader_fun, self.create_rlg = create_dataloader_fun, create_rlg
        self.max_depth = max_depth
        self.minibatch_default, self.minibatch_overrides = minibatch_default, minibatch_overrides
        self.tick_kimg_default, self.tick_kimg_overrides = tick_kimg_default, tick_kimg_overrides
        self.lod_training_nimg, self.lod_transition_nimg = lod_training_nimg, lod_transition_nimg
        self.max_lod, self.depth_offset = max_lod, depth_offset      # only for the 'lod' statistic of the original paper
        self.trainer = None
        self.depth = self.alpha = -1                                 # "nothing applied yet"

    @property
    def _reports_lod(self):
        return self.max_lod is not None and self.depth_offset is not None

    @property
    def lod(self):
        return self.max_lod - self.depth_offset - self.depth - self.alpha + 1 if self._reports_lod else -1

    def schedule(self, cur_nimg):
        return growth_stage(cur_nimg, self.lod_training_nimg, self.lod_transition_nimg, self.max_depth)

    def register(self, trainer):
        self.trainer = trainer
        stats = trainer.stats
        stats['minibatch_size'] = self.minibatch_default
        _stat(stats, 'alpha', self.alpha)
        if self._reports_lod:
            _stat(stats, 'lod', self.lod)
        self.iteration()                                             # stage 0 is applied before the first step

    def _enter_stage(self, depth):
        tr = self.trainer
        for target in (tr.D, tr.G):
            target.depth = depth
        tr.dataset.model_depth = depth
        self.depth = depth
        batch = self.minibatch_overrides.get(depth, self.minibatch_default)
        tr.dataiter = iter(self.create_dataloader_fun(batch))
        tr.random_latents_generator = self.create_rlg(batch)
        tr.tick_duration_nimg = 1000 * self.tick_kimg_overrides.get(depth, self.tick_kimg_default)
        tr.stats['minibatch_size'] = batch

    def _set_alpha(self, alpha):
        tr = self.trainer
        for target in (tr.D, tr.G, tr.dataset):
            target.alpha = alpha
        self.alpha = alpha

    def iteration(self, *args):
        tr = self.trainer
        depth, alpha = self.schedule(tr.cur_nimg)
        if depth != self.depth:
            self._enter_stage(depth)
        if alpha != self.alpha:
            self._set_alpha(alpha)
        tr.stats['depth'] = depth
        tr.stats['alpha']['val'] = alpha
        if self._reports_lod:
            tr.stats['lod']['val'] = self.lod


class LRScheduler(Plugin):
    """Steps both learning-rate schedules with the image counter after every iteration and once at registration
    (reference plugins.py:84-99); the schedulers only need ``step(cur_nimg)``."""

    def __init__(self, lr_scheduler_d, lr_scheduler_g):
        super(LRScheduler, self).__init__([(1, 'iteration')])
        self.lrs_d, self.lrs_g = lr_scheduler_d, lr_scheduler_g

    def register(self, trainer):
        self.trainer = trainer
        self.iteration()

    def iteration(self, *args):
        shown = self.trainer.cur_nimg
        for sched in (self.lrs_d, self.lrs_g):
            sched.step(shown)


class RampupLR(object):
    """``LambdaLR(opt, rampup).step(cur_nimg)`` without the scheduler machinery: sets
    ``lr = base_lr * fn(cur_nimg)`` on every param group (what plugins.py:97-99 drives).  Like torch's
    schedulers the base rate is kept in the group as ``initial_lr``, so it survives an optimizer
    state_dict round trip (a resumed run must not ramp from the already-ramped rate)."""

    def __init__(self, optimizer, fn):
        self.optimizer, self.fn = optimizer, fn
        for g in optimizer.param_groups:
            g.setdefault('initial_lr', g['lr'])
        self.base_lrs = [g['initial_lr'] for g in optimizer.param_groups]

    def step(self, cur_nimg):
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g['lr'] = base * self.fn(cur_nimg)


class TimeMonitor(Plugin):
    """Per-tick timing stats under the reference's names (plugins.py:114-139: ``stats['time']``, ``stats['sec']['tick']``,
    ``stats['sec']['kimg']``) plus the two numbers this project's benchmark is quoted in: ``stats['img/s']`` (images shown per
    second over the tick, all ranks) and ``stats['d_gp_ms']`` (device time of the D step + gradient penalty + Adam(D), mean of the
    sampled iterations of the tick; ``Trainer`` brackets every ``sample_every``-th D update with two HIP events on the streams it
    runs on).  The device is synchronised at tick boundaries only -- the host clock is the device's there and nowhere else."""

    stat_name = 'time'

    def __init__(self, base_time=0, sample_every=16):
        super(TimeMonitor, self).__init__([(1, 'epoch')])
        self.base_time = base_time
        self.sample_every = int(sample_every)

    def register(self, trainer):
        self.trainer = trainer
        self.start_time = self.epoch_start = time.time()
        self.start_nimg = trainer.cur_nimg
        trainer.stats['sec'] = {'log_format': ':.1f'}
        _stat(trainer.stats, 'img/s', 0.0, '{val:.1f}')
        _stat(trainer.stats, 'd_gp_ms', 0.0, '{val:.3f}')
        trainer.d_step_probe = dict(every=max(1, self.sample_every), pairs=[])

    def epoch(self, epoch_index):
        import torch
        tr = self.trainer
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        now = time.time()
        tick_time = now - self.epoch_start
        self.epoch_start = now
        nimg = max(1, tr.cur_nimg - self.start_nimg)
        self.start_nimg = tr.cur_nimg
        tr.stats['time'] = timedelta(seconds=now - self.start_time + self.base_time)
        tr.stats['sec']['tick'] = tick_time
        tr.stats['sec']['kimg'] = tick_time / nimg * 1000
        tr.stats['img/s']['val'] = nimg / max(tick_time, 1e-9)
        probe = getattr(tr, 'd_step_probe', None)
        if probe and probe['pairs']:
            ms = [a.elapsed_time(b) for a, b in probe['pairs']]
            tr.stats['d_gp_ms']['val'] = sum(ms) / len(ms)
            del probe['pairs'][:]


AbsoluteTimeMonitor = TimeMonitor      # the reference's name (plugins.py:114; train.py: ``AbsoluteTimeMonitor(params['resume_time'])``): drop-in


class SaverPlugin(Plugin):
    """Network snapshots with the reference's file names and whole-module pickles (plugins.py:142-174):
    ``network-snapshot-{generator|discriminator}-{kimg:06}.dat`` every ``network_snapshot_ticks`` ticks and at
    the end.  The pickles carry the packed weights AND the equalized-lr constants ``c`` (network.py:19-20 keeps
    ``c`` outside the state_dict, so whole-module pickling is what makes a snapshot resumable).

    Addition over the reference: ``network-snapshot-trainer-{kimg:06}.dat`` with both Adam
    states and ``cur_nimg`` — the reference restarts Adam from zero moments on resume.  A trainer with a smoothed generator
    (``Trainer(g_ema=...)``) also gets ``network-snapshot-generator_smoothed-{kimg:06}.dat``, a whole-module pickle of Gs (an ordinary
    ``Generator``: ``utils.output_samples`` takes it), and ``ema_beta`` / ``ema_halflife_kimg`` in the trainer file."""

    last_pattern = 'network-snapshot-{}-{}.dat'

    def __init__(self, checkpoints_path, keep_old_checkpoints=False, network_snapshot_ticks=40):
        super(SaverPlugin, self).__init__([(network_snapshot_ticks, 'epoch'), (1, 'end')])
        self.checkpoints_path = checkpoints_path
        self.keep_old_checkpoints = keep_old_checkpoints

    def register(self, trainer):
        self.trainer = trainer

    def epoch(self, epoch_index):
        import torch
        tr = self.trainer
        if _is_replica(tr):
            return
        if not self.keep_old_checkpoints:
            self._clear(self.last_pattern.format('*', '*'))
        kimg = '{:06}'.format(tr.cur_nimg // 1000)
        models = [(tr.G, 'generator'), (tr.D, 'discriminator')]
        state = {'cur_nimg': tr.cur_nimg, 'optimizer_d': tr.optimizer_d.state_dict(),
                 'optimizer_g': tr.optimizer_g.state_dict()}
        ema = getattr(tr, 'g_ema', None)
        if ema is not None:
            models.append((ema.network(), 'generator_smoothed'))             # (network(): this stream is behind the last average)
            state.update(ema_beta=ema.beta, ema_halflife_kimg=ema.halflife_kimg)
        for model, name in models:
            torch.save(model, os.path.join(self.checkpoints_path, self.last_pattern.format(name, kimg)))
        torch.save(state, os.path.join(self.checkpoints_path, self.last_pattern.format('trainer', kimg)))

    def end(self, *args):
        self.epoch(*args)

    def _clear(self, pattern):
        for file_name in glob(os.path.join(self.checkpoints_path, pattern)):
            os.remove(file_name)


def load_models(resume_network, result_dir, logger=None):
    """reference train.py:60-64: ``resume_network`` is a pattern with one ``{}`` for generator/discriminator."""
    import torch
    if logger is not None:
        logger.log('Resuming {}'.format(resume_network))
    G = torch.load(os.path.join(result_dir, resume_network.format('generator')), weights_only=False)
    D = torch.load(os.path.join(result_dir, resume_network.format('discriminator')), weights_only=False)
    return G, D


def load_smoothed_generator(resume_network, result_dir):
    """The smoothed generator SaverPlugin wrote next to ``load_models``' pair, for ``GeneratorEMA(G, Gs=...)``; None when the snapshot has
    none (written without an average, or by an earlier version): the caller starts the average from G."""
    import torch
    path = os.path.join(result_dir, resume_network.format('generator_smoothed'))
    if not os.path.exists(path):
        return None
    return torch.load(path, weights_only=False)


def load_trainer_state(resume_network, result_dir, optimizer_d, optimizer_g):
    """Restore the Adam moments / step counts written by SaverPlugin; returns ``resume_nimg`` for Trainer."""
    import torch
    state = torch.load(os.path.join(result_dir, resume_network.format('trainer')), weights_only=False)
    optimizer_d.load_state_dict(state['optimizer_d'])
    optimizer_g.load_state_dict(state['optimizer_g'])
    return state['cur_nimg']


class Evaluation(Plugin):
    """What the per-tick evaluations share: they fire every ``ticks`` ticks and at the end, on rank 0 only (replicas are identical), as
    ``evaluate(tick)`` -- the one method a subclass writes.  ``smoothed``: None = the smoothed generator of ``Trainer(g_ema=...)`` when
    there is one, else G; False = G; True = the smoothed one, or an error at ``register``.  ``precision``: 'fp32' (default) evaluates
    that network itself, 'bf16' its ``sampling.Sampler``; ``_output_generator`` has the rule and the measured cost of 'bf16'.
    ``generator()`` is the object to call ``.forward(z)`` on, ``stat(name, value, fmt)`` writes one ``trainer.stats`` entry, and
    ``cached(key, make)`` keeps the one metric object of the current stage in ``_metric_obj``."""

    def __init__(self, ticks, smoothed=None, precision='fp32'):
        super(Evaluation, self).__init__([(ticks, 'epoch'), (1, 'end')])
        self.smoothed = smoothed
        self.precision = _check_precision(precision, type(self).__name__)
        self._metric_obj = self._metric_key = None

    def register(self, trainer):
        _check_smoothed(trainer, self.smoothed, type(self).__name__)
        self.trainer = trainer

    def epoch(self, epoch_index):
        if not _is_replica(self.trainer):
            self.evaluate(epoch_index)

    def end(self, *args):
        self.epoch(*args)

    def evaluate(self, tick):
        raise NotImplementedError

    def generator(self):
        return _output_generator(self.trainer, self.smoothed, self.precision)

    def stat(self, name, value, fmt='{val:.2f}'):
        _stat(self.trainer.stats, name, value, fmt)

    def cached(self, key, make):
        """``make()`` when ``key`` has changed, else the object made last.  One is alive at a time: the buffers of a metric are gigabytes
        at the default sizes, so a new stage drops the last stage's object BEFORE it allocates its own."""
        if self._metric_obj is None or self._metric_key != key:
            self._metric_obj = None
            self._metric_obj, self._metric_key = make(), key
        return self._metric_obj


def _batches(total, minibatch):
    """The batch sizes of ``total`` items taken ``minibatch`` at a time, in order: all ``minibatch`` but a smaller last one."""
    for start in range(0, total, minibatch):
        yield min(minibatch, total - start)


class OutputGenerator(Evaluation):
    """Sample-grid hook (plugins.py:177-195): every ``output_snapshot_ticks`` ticks run G on fresh latents and
    hand the fp32 ``[n,C,H,W]`` array to each postprocessor as ``proc(out, kimg)``.  A postprocessor exposing
    ``accepts_device_tensors`` (``utils.DeviceImageSaver``) gets the device tensor instead, so only the final
    uint8 grid crosses PCIe.  ``smoothed``, ``precision``: as in ``Evaluation``."""

    def __init__(self, sample_fn, output_postprocessors, samples_count=6, output_snapshot_ticks=3, smoothed=None, precision='fp32'):
        super(OutputGenerator, self).__init__(output_snapshot_ticks, smoothed, precision)
        self.sample_fn = sample_fn
        self.output_postprocessors = output_postprocessors
        self.samples_count = samples_count

    def evaluate(self, tick):
        from .utils import run_postprocessors
        out_dev = self.generator().forward(self.sample_fn(self.samples_count).cuda())
        run_postprocessors(out_dev, self.trainer.cur_nimg // 1000, self.output_postprocessors)


class SWDMonitor(Evaluation):
    """Quality metric per tick (``metrics.SlicedWasserstein``; the reference reports none): every ``swd_ticks`` ticks and at the end,
    ``num_images`` real images from ``real_batch_fn(n)`` (fp32 device batches ``[n,C,R,R]`` at the current stage's resolution, e.g.
    ``utils.prepare_real_batch`` of a dataset batch or ``DeviceImageDataset.metric_batches()``) are measured against as many of ``G.forward(sample_fn(n).cuda())``, ``minibatch``
    at a time -- of the smoothed generator when the trainer keeps one, which is what the paper measures (``smoothed`` as in
    ``Evaluation``).  Writes ``stats['swd']``
    (the mean over the pyramid levels, x 1000) and one ``stats['swd_<res>']`` per level under the stat-dict convention of the other monitors.  Stages below 16x16 have no pyramid level: nothing is written there.  Rank 0
    evaluates (replicas are identical).  The channel count C comes from ``G.num_channels`` (3 where ``G`` has no such attribute): three
    channels are measured by ``SlicedWasserstein``, 1, 2 and 4 -- the spectrogram networks -- by ``metrics.ChannelSlicedWasserstein``
    (unpinned, this project's extension of the paper's 7x7x3 descriptor).  ``metric_kwargs`` go to ``SlicedWasserstein`` (patches_per_image, dir_repeats,
    dirs_per_repeat, seed).  One metric object (buffers, patch centres, directions) is alive at a time: a new stage drops the last
    stage's before it allocates its own (about 20 GB at the default size and 1024x1024).

    The default period rests on an ESTIMATE, not on a measurement (docs/experiments_swd.md; the metric's own kernels have been timed
    there -- 2.6 s at 1024x1024 x 3 -- the generator passes and the real batches of an evaluation have not): 10-15 s per evaluation of 16384 images at the 1024x1024 stage, most of it the generator passes and the real
    batches.  Under 1 % of that stage's time (a tick of 1 kimg is about 3.3 s there) then needs 300-450 ticks between evaluations:
    400.  A run that wants the metric more often trades images for it (``num_images=2048, swd_ticks=50`` costs the same by the
    same estimate and is noisier).

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation``."""

    def __init__(self, real_batch_fn, sample_fn, num_images=16384, minibatch=16, swd_ticks=400, smoothed=None, precision='fp32',
                 **metric_kwargs):
        super(SWDMonitor, self).__init__(swd_ticks, smoothed, precision)
        if int(num_images) < 1 or int(minibatch) < 1:
            raise ValueError('num_images and minibatch must be positive')
        self.real_batch_fn, self.sample_fn = real_batch_fn, sample_fn
        self.num_images, self.minibatch = int(num_images), int(minibatch)
        self.metric_kwargs = metric_kwargs

    def evaluate(self, tick):
        resolution, channels = 4 * 2 ** self.trainer.G.depth, int(getattr(self.trainer.G, 'num_channels', 3))
        if resolution < 16:
            return
        if channels == 3:
            make = lambda: metrics.SlicedWasserstein(resolution, self.num_images, **self.metric_kwargs)
        else:
            make = lambda: metrics.ChannelSlicedWasserstein(resolution, self.num_images, channels, **self.metric_kwargs)
        metric = self.cached((resolution, channels), make)
        metric.reset()
        gen = self.generator()
        for n in _batches(self.num_images, self.minibatch):
            metric.feed_real(self.real_batch_fn(n))
            metric.feed_fake(gen.forward(self.sample_fn(n).cuda()))
        res = metric.result()
        self.stat('swd', res['mean'], '{val:.3f}')
        for size, value in zip(res['levels'], res['swd']):
            self.stat('swd_%d' % size, value, '{val:.3f}')


class MSSSIMMonitor(Evaluation):
    """Diversity metric per tick (``metrics.MultiScaleSSIM``; the reference reports none): every ``msssim_ticks`` ticks and at the end,
    ``num_pairs`` pairs of generated images are compared, ``minibatch`` pairs at a time.  Each round is two forward passes on
    independent latents from ``sample_fn(n).cuda()``, fed as pairs -- of the smoothed generator when the trainer keeps one (``smoothed``
    as in ``Evaluation``).  Writes
    ``stats['msssim']`` (the mean over the pairs; it RISES when the generator loses variation) and ``stats['msssim_std']`` under the
    stat-dict convention of the other monitors.  The channel count comes from ``G``: one-channel networks are measured like RGB
    ones.  Stages below 16x16 have no scale: nothing is written there.  Rank 0 evaluates (replicas are identical).
    ``metric_kwargs`` go to ``MultiScaleSSIM`` (drange, quantize).

    ``num_pairs = 10000`` is the paper's count.  The default period is BORROWED from ``SWDMonitor``'s estimate, not measured: an
    evaluation is 20 000 generator passes against the SWD's 16 384 plus its real batches, and the metric's own kernels are the small
    part; no evaluation of either has been timed on the device inside a training run.  Re-derive it as docs/experiments_swd.md
    does: ticks >= 100 x evaluation seconds / tick seconds at 1024x1024 keeps the metric under 1 % of that stage's time.

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation``."""

    def __init__(self, sample_fn, num_pairs=10000, minibatch=16, msssim_ticks=400, smoothed=None, precision='fp32', **metric_kwargs):
        super(MSSSIMMonitor, self).__init__(msssim_ticks, smoothed, precision)
        if int(num_pairs) < 1 or int(minibatch) < 1:
            raise ValueError('num_pairs and minibatch must be positive')
        self.sample_fn = sample_fn
        self.num_pairs, self.minibatch = int(num_pairs), int(minibatch)
        self.metric_kwargs = metric_kwargs

    def evaluate(self, tick):
        resolution, channels = 4 * 2 ** self.trainer.G.depth, int(self.trainer.G.num_channels)
        if resolution < 16:
            return
        metric = self.cached((resolution, channels),
                             lambda: metrics.MultiScaleSSIM(resolution, self.num_pairs, num_channels=channels, **self.metric_kwargs))
        metric.reset()
        gen = self.generator()
        for n in _batches(self.num_pairs, self.minibatch):
            a = gen.forward(self.sample_fn(n).cuda())
            metric.feed(a, gen.forward(self.sample_fn(n).cuda()))
        res = metric.result()
        self.stat('msssim', res['msssim'], '{val:.4f}')
        self.stat('msssim_std', res['std'], '{val:.4f}')


class _NeighbourSheet(Evaluation):
    """What ``NNMonitor`` and ``ShiftNNMonitor`` share: ``num_samples`` generated images are searched for their ``k`` nearest training
    items, two stats are written and the post-processors get the sheet of (k + 1)^2 images.  A subclass declares ``metric`` (the name of
    the class in ``metrics``; it is made once, with ``metric_kwargs`` on top of k, mirror and drange), ``stat_prefix`` and ``sheet_prefix`` (the
    prefixes of the stat names and of the description) and ``fields`` (the result fields ``neighbours()`` takes)."""

    metric = stat_prefix = sheet_prefix = fields = None

    def __init__(self, ticks, dataset, sample_fn, num_samples, k, postprocessors, smoothed, mirror, drange, precision, **metric_kwargs):
        super(_NeighbourSheet, self).__init__(ticks, smoothed, precision)
        self.k = _int_in(k, 1, None, 'k must be a positive integer, got %r' % (k,))
        if int(num_samples) != num_samples or int(num_samples) < self.k + 1:
            raise ValueError('num_samples = %r: the sheet shows k + 1 = %d samples' % (num_samples, self.k + 1))
        self.dataset, self.sample_fn, self.num_samples = dataset, sample_fn, int(num_samples)
        self.postprocessors = postprocessors
        self.mirror = bool(getattr(dataset, 'mirror_augment', False)) if mirror is None else bool(mirror)
        self.drange, self.metric_kwargs = drange, metric_kwargs

    def evaluate(self, tick):
        import torch
        from .utils import run_postprocessors
        nn = self.cached('all stages', lambda: getattr(metrics, self.metric)(self.dataset, k=self.k, mirror=self.mirror, drange=self.drange,
                                                                            **self.metric_kwargs))
        samples = self.generator().forward(self.sample_fn(self.num_samples).cuda())
        res = nn.search(samples)
        nearest = res['rms'][:, 0].numpy()                                 # fp64 on the host
        self.stat(self.stat_prefix + 'rms', float(nearest.mean()))
        self.stat(self.stat_prefix + 'rms_min', float(nearest.min()))
        if not self.postprocessors:
            return
        rows = self.k + 1
        near = nn.neighbours({name: res[name][:rows] for name in self.fields})                    # [rows, k, C, r, r]
        shown = samples[:rows].to(near.device)
        batch = torch.cat([shown.unsqueeze(1), near], dim=1).reshape((rows * rows,) + tuple(shown.shape[1:]))
        run_postprocessors(batch, '%s%06d' % (self.sheet_prefix, self.trainer.cur_nimg // 1000), self.postprocessors)


class NNMonitor(_NeighbourSheet):
    """Novelty check per tick (``metrics.NearestNeighbours``; the reference reports none): every ``nn_ticks`` ticks and at the end,
    ``num_samples`` images of ``G.forward(sample_fn(num_samples).cuda())`` -- of the smoothed generator when the trainer keeps one
    (``smoothed`` as in ``Evaluation``) -- are searched for their ``k`` nearest training images in ``dataset`` (a
    ``DeviceImageDataset``; the stack of the current growth stage is searched) by exact L2 distance over the 0..255 levels of the saved
    image.  Writes ``stats['nn_rms']``, the mean over the samples of the distance to the nearest training image as an RMS difference per
    byte in levels, and ``stats['nn_rms_min']``, the smallest of them -- the most suspicious sample: a value near 0 is a copy -- under the
    stat-dict convention of the other monitors.  ``mirror``: also match mirrored training images; None takes ``dataset.mirror_augment``.
    Rank 0 evaluates (replicas are identical; every rank's shard is NOT searched: the distances are to rank 0's images).

    Every post-processor gets ONE batch of (k + 1)^2 images as ``proc(batch, 'nn_%06d' % kimg)``: the first k + 1 samples, each followed
    by its k neighbours.  The image grid is ceil(sqrt(n)) = k + 1 wide, so a row of ``fakes_nn_<kimg>.png`` is a sample and, to its
    right, its nearest training images in ascending distance.  A post-processor with ``accepts_device_tensors`` gets the device tensor.

    The default period follows docs/experiments_nn.md: a pass over the stack measured 0.39 ms per GB at 1024x1024 (2.6 TB/s with 64
    queries), i.e. 36 ms for 30 000 images of 3 x 1024^2 by proportion (that size itself was not run), 64 samples and their mirrors are
    two passes, and the 64 generator passes are bounded by 64/3 measured train steps of 10.1 ms = 0.22 s; an evaluation is under 0.3 s,
    and under 1 % of a 3.3 s tick of 1 kimg (the rule of docs/experiments_swd.md) needs ticks >= 100 x 0.3 / 3.3 = 9: 10.

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation``."""

    metric, stat_prefix, sheet_prefix, fields = 'NearestNeighbours', 'nn_', 'nn_', ('index', 'mirrored')

    def __init__(self, dataset, sample_fn, num_samples=64, k=3, nn_ticks=10, postprocessors=(), smoothed=None, mirror=None,
                 drange=(-1, 1), precision='fp32'):
        super(NNMonitor, self).__init__(nn_ticks, dataset, sample_fn, num_samples, k, postprocessors, smoothed, mirror, drange, precision)


class ShiftNNMonitor(_NeighbourSheet):
    """``NNMonitor`` for strip data sets (``metrics.ShiftNearestNeighbours``): every ``nn_ticks`` ticks and at the end, ``num_samples``
    generated images are searched for their ``k`` nearest training windows over EVERY start column of the recordings of ``dataset`` (a
    ``DeviceStripDataset``; the level of the current growth stage is searched), not only the non-overlapping windows ``NNMonitor``
    sees through ``level_stack()``: a generator that has memorised a passage starting anywhere in a recording reads as a copy.
    Writes ``stats['nn_shift_rms']``, the mean over the samples of the distance to the nearest window as an RMS difference per byte in
    levels, and ``stats['nn_shift_rms_min']``, the smallest of them.  ``mirror``: also match time-reversed windows; None takes
    ``dataset.mirror_augment``.  ``seg``: starts per segment (one neighbour is reported per segment; default the window width).
    Rank 0 evaluates (replicas are identical; every rank's shard is NOT searched).

    Every post-processor gets ONE batch of (k + 1)^2 images as ``proc(batch, 'nnshift_%06d' % kimg)``, laid out as ``NNMonitor``'s
    sheet: a row is a sample and, to its right, its nearest training windows in ascending distance.  A sound saver among the
    post-processors therefore also writes the neighbours' audio.

    The default period follows docs/experiments_shiftnn.md: a pass of 64 queries over 10 minutes of two-channel sound (10 strips x 75 000
    columns) measured 195 ms at S = 1024 (12.7 ms at S = 256), 64 samples are one pass (two with mirror matching), and the 64 generator
    passes are bounded by 64/3 measured train steps of 10.1 ms = 0.22 s; an evaluation is under 0.61 s even with mirror matching, and
    under 1 % of a 3.3 s tick of 1 kimg (the rule of docs/experiments_swd.md) needs ticks >= 100 x 0.61 / 3.3 = 18.5: 20.  The search
    is proportional to the length of the recordings: an hour of them costs six times as much, and ``nn_ticks`` should grow with it.

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation``."""

    metric, stat_prefix, sheet_prefix, fields = 'ShiftNearestNeighbours', 'nn_shift_', 'nnshift_', ('strip', 'start', 'mirrored')

    def __init__(self, dataset, sample_fn, num_samples=64, k=3, nn_ticks=20, postprocessors=(), smoothed=None, mirror=None,
                 drange=(-1, 1), precision='fp32', seg=None):
        super(ShiftNNMonitor, self).__init__(nn_ticks, dataset, sample_fn, num_samples, k, postprocessors, smoothed, mirror, drange, precision,
                                             seg=seg)
        self.seg = seg


class _FittedSamples(Evaluation):
    """What ``NDBMonitor``, ``PRDMonitor``, ``FDMonitor`` and ``KIDMonitor`` share: one metric object for all stages, fitted on ``dataset`` again when the stage's
    resolution differs from the fitted one, then fed ``num_samples`` generated images ``minibatch`` at a time.  A subclass writes
    ``make_metric()`` (a ``fit()`` / ``reset()`` / ``feed()`` / ``result()`` metric with ``resolution``) and ``write_stats(result)``."""

    def __init__(self, ticks, dataset, sample_fn, num_samples, minibatch, smoothed, precision):
        super(_FittedSamples, self).__init__(ticks, smoothed, precision)
        if int(num_samples) < 1 or int(minibatch) < 1:
            raise ValueError('num_samples and minibatch must be positive')
        self.dataset, self.sample_fn = dataset, sample_fn
        self.num_samples, self.minibatch = int(num_samples), int(minibatch)

    def _stage_resolution(self):
        stage = getattr(self.dataset, '_stage', None)
        if stage is None:
            return int(self.dataset.level_stack().shape[-1])
        _, shift, depthdiff = stage()                                        # (no level is made for the answer)
        return int(self.dataset.shape[-1]) >> (shift + depthdiff)

    def evaluate(self, tick):
        metric = self.cached('all stages', self.make_metric)
        if metric.resolution != self._stage_resolution():
            metric.fit()                                                     # (once per stage: the fit is retaken, the object stays)
        metric.reset()
        gen = self.generator()
        for n in _batches(self.num_samples, self.minibatch):
            metric.feed(gen.forward(self.sample_fn(n).cuda()))
        self.write_stats(metric.result())


class NDBMonitor(_FittedSamples):
    """Mode-coverage metric per tick (``metrics.NDB``: NDB/k and the JS divergence over k-means bins of the training images; the
    reference reports none): every ``ndb_ticks`` ticks and at the end, ``num_samples`` images of ``G.forward(sample_fn(n).cuda())``,
    ``minibatch`` at a time -- of the smoothed generator when the trainer keeps one (``smoothed`` as in ``Evaluation``) -- are counted
    per bin and compared with the proportions of held-out training images.  ``dataset``: a ``DeviceImageDataset``; the bins are
    fitted on ``level_stack()`` of the current growth stage and REFITTED when the stage's resolution differs from the fitted one (a
    fit happens once per stage, not per evaluation).  ``holdout=None`` holds out ``min(M // 5, num_samples)`` training images for the
    reference proportions (``metrics.NDB`` says why a hold-out is the form to use); ``k`` bins, at most ``ops.NN_MAX_QUERIES``.
    Writes ``stats['ndb']`` (the number of bins whose two proportions differ at the 5 % level), ``stats['ndb_over_k']`` and
    ``stats['jsd']`` under the stat-dict convention of the other monitors.  Defined per image vector: one-channel networks are measured
    like RGB ones.  Rank 0 evaluates (replicas are identical; the bins are rank 0's shard).  Opt-in: a run that does not register it
    pays nothing.  ``metric_kwargs`` go to ``NDB`` (seed, max_iter, z_threshold, drange).

    The default period follows docs/experiments_ndb.md: the metric's own part of an evaluation of 8192 samples measured 0.07 s at 3x1024^2
    (512 batches of 16 against 50 centroids), the fit 0.70 ms per GB of stack and iteration, i.e. at most 30 x 66 ms = 2.0 s for 30 000
    images of 3x1024^2 by proportion (that size itself was not run), once per stage; the 8192 generator passes are bounded by 8192 images
    at the 296 img/s of a whole measured train step, 27.7 s.  An evaluation is under 27.8 s, and under 1 % of a 3.3 s tick of 1 kimg (the
    rule of docs/experiments_swd.md) needs ticks >= 100 x 27.8 / 3.3 = 842: 850.  ``num_samples=2048, ndb_ticks=200`` costs the same
    share with a noisier histogram.

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation``."""

    def __init__(self, dataset, sample_fn, num_samples=8192, minibatch=16, k=50, holdout=None, ndb_ticks=850, smoothed=None,
                 precision='fp32', **metric_kwargs):
        super(NDBMonitor, self).__init__(ndb_ticks, dataset, sample_fn, num_samples, minibatch, smoothed, precision)
        self.k = k
        self.holdout = min(len(dataset) // 5, self.num_samples) if holdout is None else holdout
        self.metric_kwargs = metric_kwargs

    def make_metric(self):
        return metrics.NDB(self.dataset, k=self.k, holdout=self.holdout, **self.metric_kwargs)

    def write_stats(self, res):
        self.stat('ndb', res['ndb'], '{val:d}')
        self.stat('ndb_over_k', res['ndb_over_k'], '{val:.3f}')
        self.stat('jsd', res['jsd'], '{val:.4f}')


class PRDMonitor(_FittedSamples):
    """Fidelity and coverage per tick as separate numbers (``metrics.PrecisionRecall``: improved precision and recall over k-NN balls
    with density and coverage, in uint8 image space; the reference reports none): every ``prd_ticks`` ticks and at the end,
    ``num_samples`` images of ``G.forward(sample_fn(n).cuda())``, ``minibatch`` at a time -- of the smoothed generator when the trainer
    keeps one (``smoothed`` as in ``Evaluation``) -- against ``num_real`` training images (``metric_kwargs``; default: all).
    ``dataset``: a ``DeviceImageDataset`` or a ``DeviceStripDataset``; the reals and their radii are taken from ``level_stack()`` of the
    current growth stage and REFITTED when the stage's resolution differs from the fitted one (once per stage, not per evaluation).
    Writes ``stats['precision']``, ``stats['recall']``, ``stats['density']`` and ``stats['coverage']`` under the stat-dict convention of
    the other monitors.  Defined per image vector: one-channel networks are measured like RGB ones.  Rank 0 evaluates (replicas are
    identical; the reals are rank 0's shard).  Opt-in: a run that does not register it pays nothing.  ``metric_kwargs`` go to
    ``PrecisionRecall`` (num_real, max_resolution, seed, drange).

    ``max_resolution`` defaults to 256 HERE (``PrecisionRecall`` itself keeps the stage's resolution): above 256^2 both sets are
    reduced with ``ops.pyramid_level_u8`` before they are compared.  The tile kernel gives every 128 x 128 tile of pairs to one
    workgroup for all of D, so a few thousand images of 3 x 1024^2 bytes leave most of the device idle (docs/experiments_prd.md: 1024
    against 1024 at 3 x 1024^2 took 23.6 ms and 25.4 ms per pass, 0.73x and 0.68x the composition from ``ops.l2dist_u8``), while at
    3 x 256^2 and below the fused passes measured 2.9x to 40x faster than that composition.

    The defaults follow docs/experiments_prd.md: with 4096 samples against 4096 reals the metric's own part of an evaluation measured
    0.007 s at 1 x 256^2 (feed 2.9 ms for 256 batches of 16, the radii of the fakes and the ball pass 3.7 ms with the host read) and
    the fit 2.0 ms; at 3 x 256^2 a radii pass over 4096 images took 6.2 ms and the ball pass 4096 x 4096 6.2 ms, i.e. for 30 000
    reals by proportion (that size itself was not run) 6.2 x (30000 / 4096)^2 = 0.33 s for the fit, once per stage, and
    6.2 + 6.2 x 30000 / 4096 = 52 ms per evaluation.  The 4096 generator passes are bounded by 4096 images at the 296 img/s of a
    whole measured train step at 1024^2, 13.8 s.  An evaluation is under 13.8 + 0.1 + 0.33 = 14.3 s, and under 1 % of a 3.3 s tick of
    1 kimg (the rule of docs/experiments_swd.md) needs ticks >= 100 x 14.3 / 3.3 = 433: 450.  ``num_samples=1024, prd_ticks=110``
    costs the same share with noisier numbers; k-NN statistics need both sets in the thousands to be stable.

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation`` (unrelated to the statistic of that name)."""

    def __init__(self, dataset, sample_fn, num_samples=4096, minibatch=16, k=3, prd_ticks=450, smoothed=None, precision='fp32',
                 **metric_kwargs):
        super(PRDMonitor, self).__init__(prd_ticks, dataset, sample_fn, num_samples, minibatch, smoothed, precision)
        self.k = _int_in(k, 1, self.num_samples - 1, 'k = %r for %d samples (the radii of the samples need k + 1 of them)' % (k, num_samples))
        self.metric_kwargs = dict(metric_kwargs)
        self.metric_kwargs.setdefault('max_resolution', 256)

    def make_metric(self):
        return metrics.PrecisionRecall(self.dataset, k=self.k, **self.metric_kwargs)

    def write_stats(self, res):
        for name in ('precision', 'recall', 'density', 'coverage'):
            self.stat(name, res[name], '{val:.3f}')


class FDMonitor(_FittedSamples):
    """The Frechet distance ``fd`` per tick (``metrics.FrechetDistance``: the distance between the feature moments of training and
    generated images over a randomly initialised convolutional embedding; the reference reports none): every ``fd_ticks`` ticks and at
    the end, ``num_samples`` images of ``G.forward(sample_fn(n).cuda())``, ``minibatch`` at a time -- of the smoothed generator when the
    trainer keeps one (``smoothed`` as in ``Evaluation``) -- against ``num_real`` training images (``metric_kwargs``; default: all).
    ``dataset``: a ``DeviceImageDataset`` or a ``DeviceStripDataset``; the reals are embedded from ``level_stack()`` of the current
    growth stage and REFITTED when the stage's resolution differs from the fitted one (once per stage, not per evaluation).  Writes
    ``stats['fd']`` under the stat-dict convention of the other monitors.  It is NOT the Inception distance (FID): comparable between
    runs of this project, not with published tables.  1- to 4-channel networks are measured alike.  Rank 0 evaluates (replicas are
    identical; the reals are rank 0's shard).  Opt-in: a run that does not register it pays nothing.  ``metric_kwargs`` go to
    ``FrechetDistance`` (num_real, max_resolution, seed, drange, embedding); above ``max_resolution`` = 256 both sets are reduced with
    ``ops.pyramid_level_u8`` before they are embedded.

    The default period follows docs/experiments_fd.md, from one run that timed the generator passes and the metric together (a default
    generator, batches of 16, 512 samples timed and scaled): at 3x1024^2 the 4096 generator passes took 0.66 s, feeding them (quantise,
    reduce to 256^2, embed: 256 batches of 16) 0.08 s more, ``result()`` (the moments of 4096 x 128 features, the host read, the
    eigenvalues) 0.004 s; the fit measured 0.010 ms per real, i.e. 0.30 s for 30 000 reals by proportion (1024 were timed), once per
    stage.  At 1x256^2: 0.39 s, 0.07 s, 0.003 s and 0.008 ms per real.  An evaluation is under 0.66 + 0.08 + 0.01 + 0.30 = 1.05 s, and
    under 1 % of a 3.3 s tick of 1 kimg (the rule of docs/experiments_swd.md) needs ticks >= 100 x 1.05 / 3.3 = 32: 40.  The metric's
    own part is an eighth of the evaluation; the rest is the generator.  A moment estimate over 128 features needs thousands of samples
    per side; ``num_samples=1024, fd_ticks=10`` costs the same share with a noisier, more biased value.

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation``."""

    def __init__(self, dataset, sample_fn, num_samples=4096, minibatch=16, fd_ticks=40, smoothed=None, precision='fp32',
                 **metric_kwargs):
        super(FDMonitor, self).__init__(fd_ticks, dataset, sample_fn, num_samples, minibatch, smoothed, precision)
        if self.num_samples < 2:
            raise ValueError('num_samples = %r (a covariance needs at least 2 samples)' % (num_samples,))
        self.metric_kwargs = dict(metric_kwargs)

    def make_metric(self):
        return metrics.FrechetDistance(self.dataset, **self.metric_kwargs)

    def write_stats(self, res):
        self.stat('fd', res['fd'], '{val:.4f}')


class KIDMonitor(_FittedSamples):
    """The kernel distance ``kid`` per tick (``metrics.KernelDistance``: the unbiased estimator of the squared maximum mean discrepancy
    between training and generated images, cubic polynomial kernel, over the randomly initialised convolutional embedding of ``fd``; the
    reference reports none): every ``kid_ticks`` ticks and at the end, ``num_samples`` images of ``G.forward(sample_fn(n).cuda())``,
    ``minibatch`` at a time -- of the smoothed generator when the trainer keeps one (``smoothed`` as in ``Evaluation``) -- against
    ``num_real`` training images (``metric_kwargs``; default: all).  ``dataset``: a ``DeviceImageDataset`` or a ``DeviceStripDataset``;
    the reals are embedded from ``level_stack()`` of the current growth stage and REFITTED when the stage's resolution differs from the
    fitted one (once per stage, not per evaluation).  Writes ``stats['kid']``, ``stats['kid_std']`` (the sample standard deviation over
    the subsets of ``subset_size`` rows) when there are at least 2 subsets, and ``stats['fd']`` with ``with_fd=True`` -- then one set of
    generator passes and one embedding serve both numbers -- under the stat-dict convention of the other monitors.  It is NOT the
    Inception-feature KID: comparable between runs of this project, not with published tables; it is not clamped at 0.  1- to 4-channel
    networks are measured alike.  Rank 0 evaluates (replicas are identical; the reals are rank 0's shard).  Opt-in: a run that does
    not register it pays nothing.  ``metric_kwargs`` go to ``KernelDistance`` (num_real, max_resolution, seed, drange, embedding,
    subset_size, gamma, coef0, with_fd); above ``max_resolution`` = 256 both sets are reduced with ``ops.pyramid_level_u8`` before they
    are embedded.

    ``num_samples`` has no floor beyond 2: the estimator is unbiased at any count, which is why this monitor exists beside
    ``FDMonitor`` -- on a data set of a few hundred recordings ``num_samples=256`` against all reals is a usable number (noisy, centred
    on the true value), where ``fd`` of the same sets is dominated by its bias.

    The default period follows docs/experiments_kid.md and the measurements of docs/experiments_fd.md, whose generator passes and
    embedding are this monitor's: at 3x1024^2 the 4096 generator passes took 0.66 s and feeding them 0.08 s; the fit is the embedding's
    0.010 ms per real, 0.30 s for 30 000 reals by proportion, once per stage, plus the reals' tile sums, which measured 0.003 s for
    30 000 reals.  What is new per evaluation is ``result()``: the self sums of 4096 fed features, the cross sums of 30 000 x 4096, the
    host read and the statistic measured 0.001 s together.  An evaluation is under 0.66 + 0.08 + 0.001 + 0.30 + 0.003 = 1.04 s, and
    under 1 % of a 3.3 s tick of 1 kimg (the rule of docs/experiments_swd.md) needs ticks >= 100 x 1.04 / 3.3 = 32: 40, the period of
    ``FDMonitor``.  The statistic's own part is 0.4 % of the evaluation; the rest is the generator and the embedding.
    ``num_samples=1024, kid_ticks=10`` costs the same share.

    ``precision``: 'fp32' (default) or 'bf16', as in ``Evaluation``."""

    def __init__(self, dataset, sample_fn, num_samples=4096, minibatch=16, kid_ticks=40, smoothed=None, precision='fp32',
                 **metric_kwargs):
        super(KIDMonitor, self).__init__(kid_ticks, dataset, sample_fn, num_samples, minibatch, smoothed, precision)
        if self.num_samples < 2:
            raise ValueError('num_samples = %r (the estimator needs at least 2 samples)' % (num_samples,))
        self.metric_kwargs = dict(metric_kwargs)

    def make_metric(self):
        return metrics.KernelDistance(self.dataset, **self.metric_kwargs)

    def write_stats(self, res):
        self.stat('kid', res['kid'], '{val:.6f}')
        if res['kid_subset_std'] is not None:
            self.stat('kid_std', res['kid_subset_std'], '{val:.6f}')
        if 'fd' in res:
            self.stat('fd', res['fd'], '{val:.4f}')


class ProjectionMonitor(Evaluation):
    """Recall-style measure per tick (``projection.Projector``; the reference reports none): every ``projection_ticks`` ticks and at the
    end, a FIXED set of ``num_images`` real images is projected into the latent space of the generator -- of the smoothed generator when
    the trainer keeps one (``smoothed`` as in ``Evaluation``) -- and the
    pyramid loss the search ends at says how well the generator can reproduce images it was not asked to produce.  It is defined for
    1-, 2-, 3- and 4-channel networks alike.

    ``source``: a ``DeviceImageDataset`` or ``DeviceStripDataset`` -- the targets are its LAST ``num_images`` items (``dataset.items``)
    at the current growth stage with alpha 1 and no mirror, the same indices at every evaluation (the end of the stack, where
    ``metrics.NDB`` holds images out as well; the training stream is not moved) -- or ``real_batch_fn(n)`` -> fp32 device batch ``[n,C,r,r]`` at the current stage's resolution, called ONCE per
    resolution and kept (give it a seeded stream of its own, e.g. ``dataset.metric_batches(seed)``).  ``projector_kwargs`` go to
    ``Projector`` (lr, betas, level_weights, seed).

    Writes ``stats['proj_loss']`` (the mean over the targets of the final loss) and ``stats['proj_loss_max']`` (the worst target)
    under the stat-dict convention of the other monitors.  With ``samples_path`` it writes ``proj_<kimg>.png`` there through
    ``utils.DeviceImageSaver``'s grid path (``drange``, ``resolution`` as there): ONE batch of 2 x num_images images, each target followed
    by its reconstruction, so that with an even grid width (ceil(sqrt(2 num_images)): 4 for the default 8) a target stands beside its
    reconstruction.  Every post-processor gets the same batch as ``proc(batch, 'proj_%06d' % kimg)``.  Rank 0 evaluates (replicas are
    identical).  Opt-in: a run that does not register it pays nothing.  ``precision='bf16'`` is refused: the bf16 sampler has no
    backward pass.

    The defaults follow docs/experiments_projection.md: a 200-step projection of 8 images measured 0.89 s at the 1024x1024 stage (4.47 ms
    per step) and 0.47 s at 256x256 (2.37 ms per step) on an MI355X, untrained weights.  Under 1 % of a 3.3 s tick of 1 kimg at 1024x1024
    (the rule of docs/experiments_swd.md) needs ticks >= 100 x 0.89 / 3.3 = 27.1: 30.  200 steps is where the search was measured; on the
    untrained networks it takes the loss of the generator's own images to 0.14 - 0.26 of the start value, a trained one was not run."""

    def __init__(self, source, num_images=8, steps=200, projection_ticks=30, smoothed=None, precision='fp32', samples_path=None,
                 drange=(-1, 1), resolution=512, postprocessors=(), **projector_kwargs):
        super(ProjectionMonitor, self).__init__(projection_ticks, smoothed, precision)
        if precision != 'fp32':
            raise ValueError("ProjectionMonitor(precision=%r): the projection needs the generator's backward sweep, which the bf16 "
                             "sampler does not have; only 'fp32' is taken" % (precision,))
        num_images = _int_in(num_images, 1, None, 'num_images must be a positive integer, got %r' % (num_images,))
        steps = _int_in(steps, 1, None, 'steps must be a positive integer, got %r' % (steps,))
        if not callable(source) and not (hasattr(source, 'items') and hasattr(source, '__len__')):
            raise ValueError('ProjectionMonitor: source must be a device dataset or a function n -> real batch, got %s' % type(source).__name__)
        if not callable(source) and len(source) < int(num_images):
            raise ValueError('ProjectionMonitor: %d targets from a dataset of %d images' % (num_images, len(source)))
        self.source = source
        self.num_images, self.steps = int(num_images), int(steps)
        self.samples_path, self.drange, self.resolution = samples_path, drange, resolution
        self.postprocessors = postprocessors
        self.projector_kwargs = projector_kwargs
        self._targets = {}               # resolution -> the fixed targets of that stage (real_batch_fn sources)
        self._projector = None           # (network it was made for, Projector)

    def targets(self, resolution):
        """The fixed targets at ``resolution``: the same images at every call."""
        import torch
        if not callable(self.source):
            ds = self.source
            M = len(ds)
            idx = torch.arange(M - self.num_images, M, dtype=torch.int64, device=getattr(ds, 'device', 'cpu'))
            return ds.items(idx)
        t = self._targets.get(resolution)
        if t is None:
            t = self.source(self.num_images)
            if tuple(t.shape[-2:]) != (resolution, resolution) or t.shape[0] != self.num_images:
                raise ValueError('ProjectionMonitor: real_batch_fn(%d) gave %s at the %dx%d stage'
                                 % (self.num_images, tuple(t.shape), resolution, resolution))
            self._targets = {resolution: t}                                  # (one stage's targets are alive at a time)
        return t

    def _projector_for(self, net):
        if self._projector is None or self._projector[0]() is not net:
            import weakref
            from .projection import Projector
            self._projector = (weakref.ref(net), Projector(net, steps=self.steps, **self.projector_kwargs))
        return self._projector[1]

    def evaluate(self, tick):
        import torch
        from .utils import DeviceImageSaver, run_postprocessors
        tr = self.trainer
        net = self.generator()
        targets = self.targets(4 * 2 ** int(net.depth))
        res = self._projector_for(net).project(targets)
        loss = res.loss.double().cpu()                                       # the one host synchronisation of an evaluation
        self.stat('proj_loss', float(loss.mean()), '{val:.5f}')
        self.stat('proj_loss_max', float(loss.max()), '{val:.5f}')
        if not self.postprocessors and self.samples_path is None:
            return
        batch = torch.stack([targets, res.images], dim=1).reshape((2 * targets.shape[0],) + tuple(targets.shape[1:]))
        if self.samples_path is not None:
            saver = DeviceImageSaver(self.samples_path, self.drange, self.resolution)
            saver.output_file_format = 'proj_{}.png'
            saver(batch, tr.cur_nimg // 1000)
        run_postprocessors(batch, 'proj_%06d' % (tr.cur_nimg // 1000), self.postprocessors)


class LossMonitor(Plugin):
    """The losses of a run per tick (replaces the reference's four ``EfficientLossMonitor``s, train.py:170-171 / plugins.py:102-111, which
    read every loss on the host every iteration).  ``iteration(i, *losses)`` makes ONE ``telemetry.ScalarStats.push`` of the tensors the
    trainer hands over, in ``names``' order (``Trainer`` passes G_loss, D_loss, D_real, D_fake; the per-sample ``[N, 1]`` losses count
    with their mean, as in the reference): one library call, no host synchronisation -- the host keeps running ahead of the device.
    ``epoch`` makes one ``read`` (a copy of K x 64 bytes; the tick boundary waits for the device anyway) and writes, for every name,
    ``stats[name]`` under the stat-dict convention of the other monitors (``log_name``, ``log_epoch_fields=['{val:.4f}']``, ``val`` = the mean
    over the tick's iterations) plus the legacy monitor's ``last`` and ``epoch_mean`` and ``min``, ``max``, ``std``, ``count``, ``nonfinite``,
    ``first_bad``.  The statistics start afresh with every tick; ``end`` reports what a last, unfinished tick has gathered.  A NaN or
    infinite loss is counted, never averaged; ``HealthMonitor`` turns it into an error.

    Stream order: the push runs on the stream that is current when the trainer calls its plugins -- the stream the loss
    functions were called on.  Eagerly, the loss block is the last launch of the forward schedule on that stream; a replayed step
    (launch plan or hipGraph) hands out copies of its reused loss buffer made on that stream after the replay.  Either way the
    push is behind the producer, and the tensors it reads are the caller's own, so the next replay cannot overwrite them.
    Host tensors or Python floats from a foreign loss go through the numpy twin.  Every rank keeps its own record."""

    def __init__(self, names=('G_loss', 'D_loss', 'D_real', 'D_fake')):
        super(LossMonitor, self).__init__([(1, 'iteration'), (1, 'epoch'), (1, 'end')])
        from .telemetry import ScalarStats
        self.scalars = ScalarStats(names)
        self.names = self.scalars.names
        self.last = None                 # (tick index, ScalarStats.read result) of the last report

    def register(self, trainer):
        self.trainer = trainer
        trainer.loss_monitor = self      # HealthMonitor looks here
        for name in self.names:
            _stat(trainer.stats, name, float('nan'), '{val:.4f}', last=float('nan'), epoch_mean=float('nan'))

    def iteration(self, i, *losses):
        if len(losses) < len(self.names):
            raise ValueError('LossMonitor: the trainer handed over %d values for %r' % (len(losses), self.names))
        self.scalars.push(*losses[:len(self.names)])

    def epoch(self, epoch_index):
        res = self.scalars.read(reset=True)
        self.last = (epoch_index, res)
        for name in self.names:
            r = res[name]
            _stat(self.trainer.stats, name, r['mean'], '{val:.4f}', last=r['last'], epoch_mean=r['mean'], min=r['min'], max=r['max'],
                  std=r['std'], count=r['count'], nonfinite=r['nonfinite'], first_bad=r['first_bad'])

    def end(self, *args):
        if not self.scalars.empty:                                       # (iterations since the last tick closed)
            self.epoch(*args)


class HealthMonitor(Evaluation):
    """Numerical guard and per-layer norms of D and G (the reference has neither): every ``health_ticks`` ticks and at the end, after
    ``engine.wait_pending(net)``, ONE ``telemetry.SegmentStats.measure`` of each network's flat parameters and -- when its optimizer is a
    ``FusedAdam`` -- one of Adam's first moment (``FusedAdam.flat_moments``), segmented into the weight and the bias of every layer.  With a
    ``torch.optim`` optimizer only the weights are measured.  Writes, under the stat-dict convention of the other monitors,
    ``stats['G_wnorm' | 'D_wnorm']`` (the L2 norm over all segments), ``stats['G_gnorm' | 'D_gnorm']`` and ``stats['G_gmax' | 'D_gmax']`` (L2
    norm and largest magnitude of the first moment).  The g-statistics equal those of the last gradient x ``grad_scale`` EXACTLY when
    beta1 = 0 (the reference's Adam: train.py:148-149); with any other beta1 they are those of Adam's running gradient average.
    ``per_layer=True`` adds one stat per layer (``'G_wnorm/blocks.3.c1.weight'`` ...); ``report()`` returns the whole table of the last
    evaluation as a list of dicts (net, layer, offset, length, wnorm, wmax, w_nonfinite, gnorm, gmax, g_nonfinite).

    On any NaN / +-Inf element in a parameter or moment segment, or any non-finite push of a registered ``LossMonitor`` in the tick,
    ``on_nonfinite='raise'`` raises ``telemetry.TrainingDiverged`` and ``'warn'`` warns (RuntimeWarning); the message names the network,
    every affected layer with its count, the loss with ``first_bad``, and the kimg.  Register it BEFORE ``SaverPlugin``: plugins due at the
    same tick fire in registration order, so the guard fires first and the poisoned snapshot is never written.  Rank 0 evaluates
    (replicas are identical)."""

    def __init__(self, health_ticks=1, on_nonfinite='raise', per_layer=False):
        super(HealthMonitor, self).__init__(health_ticks)                # (it evaluates no generator: ``smoothed`` / ``precision`` stay unused)
        if on_nonfinite not in ('raise', 'warn'):
            raise ValueError("on_nonfinite must be 'raise' or 'warn', got %r" % (on_nonfinite,))
        self.on_nonfinite, self.per_layer = on_nonfinite, bool(per_layer)
        self._seg = {}                   # net name -> (flat buffer address, SegmentStats)
        self._table = []

    def report(self):
        return [dict(row) for row in self._table]

    def _segments(self, which, net):
        from .telemetry import SegmentStats
        hit = self._seg.get(which)
        if hit is None or hit[0] != net._flat_param.data_ptr():
            hit = self._seg[which] = (net._flat_param.data_ptr(), SegmentStats.for_network(net))
        return hit[1]

    def evaluate(self, epoch_index):
        tr = self.trainer
        from . import engine
        from .telemetry import TrainingDiverged
        fmt = '{val:.4g}'
        table, problems = [], []
        for which, net, opt in (('D', tr.D, tr.optimizer_d), ('G', tr.G, tr.optimizer_g)):
            flat = getattr(net, '_flat_param', None)
            if flat is None:
                continue                                                 # a foreign network: nothing to segment
            if flat.is_cuda:
                engine.wait_pending(net)                                 # a deferred update of this network (second stream)
            seg = self._segments(which, net)
            w = seg.measure(flat)
            moments = opt.flat_moments(net) if hasattr(opt, 'flat_moments') else None
            g = seg.measure(moments[0]) if moments is not None else None
            w = w.cpu().numpy()
            g = g.cpu().numpy() if g is not None else None
            self.stat(which + '_wnorm', math.sqrt(float(w[:, 1].sum())), fmt)
            if g is not None:
                self.stat(which + '_gnorm', math.sqrt(float(g[:, 1].sum())), fmt)
                self.stat(which + '_gmax', float(g[:, 2].max()), fmt)
            bad = []
            for i, (name, (off, n)) in enumerate(zip(seg.names, seg.segments)):
                row = dict(net=which, layer=name, offset=off, length=n, wnorm=math.sqrt(float(w[i, 1])), wmax=float(w[i, 2]),
                           w_nonfinite=int(w[i, 3]), gnorm=None, gmax=None, g_nonfinite=None)
                if g is not None:
                    row.update(gnorm=math.sqrt(float(g[i, 1])), gmax=float(g[i, 2]), g_nonfinite=int(g[i, 3]))
                table.append(row)
                if self.per_layer:
                    for key in ('wnorm', 'gnorm'):
                        if row[key] is not None:
                            self.stat('%s_%s/%s' % (which, key, name), row[key], fmt)
                if row['w_nonfinite']:
                    bad.append('%s: %d of %d weights' % (name, row['w_nonfinite'], n))
                if row['g_nonfinite']:
                    bad.append('%s: %d of %d first-moment elements' % (name, row['g_nonfinite'], n))
            if bad:
                problems.append('%s has non-finite values in %s' % (which, '; '.join(bad)))
        self._table = table
        lm = getattr(tr, 'loss_monitor', None)
        if lm is not None:
            # this tick's report when the loss monitor has already fired (it was registered first), else a look at its record
            res = lm.last[1] if lm.last is not None and lm.last[0] == epoch_index and lm.scalars.empty else lm.scalars.read(reset=False)
            for name in lm.names:
                if res[name]['nonfinite']:
                    problems.append('loss %s was non-finite in %d iterations of this tick, first_bad = %d (last value %r)'
                                    % (name, res[name]['nonfinite'], res[name]['first_bad'], res[name]['last']))
        if problems:
            msg = 'training diverged at %.3f kimg (tick %s): %s' % (tr.cur_nimg / 1000., epoch_index, '. '.join(problems))
            if self.on_nonfinite == 'raise':
                raise TrainingDiverged(msg)
            warnings.warn(msg, RuntimeWarning)


class AugmentController(Plugin):
    """Adaptive augmentation probability (Karras et al. 2020, "Training GANs with limited data"): steers ``augmenter.p`` so that the
    overfitting signal ``r_t = E[sign(D(real))]`` stays at ``target``.  The D steps of an Augmenter with a controller count the signs of the
    real scores into its 16-byte device accumulator (pg_score_signs, one launch behind the loss block); every ``interval`` iterations this
    plugin reads it -- the only host synchronisation the feature adds --, forms ``r_t`` over the scores since the last read and moves
    ``p`` by ``sign(r_t - target) * images since the last read / (1000 * adjust_kimg)``, clipped to ``[0, p_max]``: ``p`` can cross [0, 1] in
    ``adjust_kimg`` thousand images.  ``p_max`` defaults to 0.8: above it flips and cutouts begin to leak into what G learns (DESIGN.md
    section 7).  Writes ``augment_p`` and ``augment_rt`` into ``trainer.stats``.  A new ``p`` enters the next table draw; no plan is
    re-recorded.  Under data parallelism every rank steers the ``p`` of its own Augmenter from its own shard's scores.

    Valid for the 'logistic' and 'hinge' kinds, whose decision boundary is score 0.  Under 'wgan' and 'lsgan' the drift term pins the real
    scores near 0 and their sign says nothing: ValueError here (an Augmenter already handed to such an objective) or in ``gan_losses``
    (the other order); those kinds run with a fixed ``p``."""

    def __init__(self, augmenter, target=0.6, adjust_kimg=500, interval=16, p_max=0.8):
        from .augment import Augmenter
        from .gan_losses import SIGN_KINDS
        if not isinstance(augmenter, Augmenter):
            raise ValueError('AugmentController: %r is not an Augmenter' % (augmenter,))
        if augmenter.kind is not None and augmenter.kind not in SIGN_KINDS:
            raise ValueError("AugmentController: the Augmenter belongs to a %r objective; the sign of the real scores is a signal for %s "
                             'only (run it with a fixed p)' % (augmenter.kind, ' and '.join(SIGN_KINDS)))
        if augmenter.controller is not None:
            raise ValueError('AugmentController: the Augmenter already has a controller')
        target, adjust_kimg, p_max = float(target), float(adjust_kimg), float(p_max)
        if not -1.0 < target < 1.0:
            raise ValueError('AugmentController: target = %r outside (-1, 1), the open range of a mean of signs' % target)
        if not 0.0 < adjust_kimg < float('inf'):
            raise ValueError('AugmentController: adjust_kimg = %r must be positive' % adjust_kimg)
        if not 0.0 <= p_max <= 1.0:
            raise ValueError('AugmentController: p_max = %r outside [0, 1]' % p_max)
        interval = _int_in(interval, 1, None, 'AugmentController: interval')
        super(AugmentController, self).__init__([(interval, 'iteration')])
        self.augmenter, self.target, self.adjust_kimg, self.interval, self.p_max = augmenter, target, adjust_kimg, interval, p_max
        self.last = None                 # (sum of signs, scores counted, trainer.cur_nimg) at the last read
        self.r_t = float('nan')
        augmenter.controller = self

    def register(self, trainer):
        self.trainer = trainer
        self.last = self.augmenter.read() + (trainer.cur_nimg,)
        self._write()

    def _write(self):
        _stat(self.trainer.stats, 'augment_p', float(self.augmenter.p), '{val:.4f}')
        _stat(self.trainer.stats, 'augment_rt', self.r_t, '{val:.4f}')

    def iteration(self, i, *losses):
        signs, count = self.augmenter.read()
        nimg = self.trainer.cur_nimg
        d_signs, d_count, d_nimg = signs - self.last[0], count - self.last[1], nimg - self.last[2]
        if d_count > 0:                  # (no D step of this Augmenter since the last read: nothing to steer by)
            self.last = (signs, count, nimg)
            self.r_t = d_signs / d_count
            step = (self.r_t > self.target) - (self.r_t < self.target)
            self.augmenter.p = min(max(float(self.augmenter.p) + step * d_nimg / (1000.0 * self.adjust_kimg), 0.0), self.p_max)
        self._write()
