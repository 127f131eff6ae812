"""pggan-pytorch_amd — MI355X-native Progressive-GAN training path.

The reference's Python surface (Generator / Discriminator / wgan_gp_D_loss / wgan_gp_G_loss /
Trainer / DepthManager / LRScheduler) on top of hand-written gfx950 HIP kernels reached through
the C-ABI of ``libpggan_hip.so`` (``include/pggan_hip.h``).  Import as
``importlib.import_module('pggan-pytorch_amd')`` or through the root-level shim ``import pggan_amd``."""
from . import _lib, runtime, ops, engine, network, wgan_gp_loss, trainer, plugins, optim, parallel, utils, graphs, plans, sound, metrics, ema, dataset, telemetry, cluster, phase, sampling, projection, augment  # noqa: F401
from .network import Generator, Discriminator, PGConv2d  # noqa: F401
from .wgan_gp_loss import wgan_gp_D_loss, wgan_gp_G_loss  # noqa: F401
from .gan_losses import gan_losses  # noqa: F401  (the function takes the module's place as the package attribute)
from .trainer import Trainer  # noqa: F401
from .plugins import (Plugin, DepthManager, LRScheduler, RampupLR, TimeMonitor, AbsoluteTimeMonitor, SaverPlugin, OutputGenerator,  # noqa: F401
                      SWDMonitor, MSSSIMMonitor, NNMonitor, ShiftNNMonitor, NDBMonitor, PRDMonitor, FDMonitor, KIDMonitor, ProjectionMonitor, LossMonitor, HealthMonitor, AugmentController, load_models, load_smoothed_generator, load_trainer_state)
from .optim import FusedAdam  # noqa: F401
from .ema import GeneratorEMA  # noqa: F401
from .parallel import DataParallel  # noqa: F401
from .sound import SoundSaver, DeviceSoundSaver, spectrogram_u8, spectrogram_stack_u8, spectrogram_strip_u8  # noqa: F401
from .sound import ResampleTable, resample_table, resample, resampled_length, load_wav  # noqa: F401
from .phase import MelTable, mel_table, mel_analyse, mel_spectrum, mel_synthesise  # noqa: F401
from .dataset import DeviceImageDataset, DeviceStripDataset, CropStream  # noqa: F401
from .metrics import NearestNeighbours, ShiftNearestNeighbours, NDB, ChannelSlicedWasserstein, PrecisionRecall, RandomEmbedding, FrechetDistance, frechet_statistic, KernelDistance, kid_statistic  # noqa: F401
from .sampling import Sampler, sampler_for  # noqa: F401
from .projection import Projector  # noqa: F401
from .augment import Augmenter  # noqa: F401
from .utils import project_samples  # noqa: F401
from .telemetry import ScalarStats, SegmentStats, TrainingDiverged  # noqa: F401
from ._lib import PgganLibraryError, LIB_PATH  # noqa: F401

__all__ = ['Generator', 'Discriminator', 'PGConv2d', 'wgan_gp_D_loss', 'wgan_gp_G_loss', 'gan_losses', 'Trainer', 'Plugin',
           'DepthManager', 'LRScheduler', 'RampupLR', 'TimeMonitor', 'AbsoluteTimeMonitor', 'SaverPlugin', 'OutputGenerator', 'SWDMonitor', 'MSSSIMMonitor', 'NNMonitor', 'load_models',
           'load_smoothed_generator', 'load_trainer_state', 'FusedAdam', 'GeneratorEMA', 'DataParallel', 'SoundSaver', 'DeviceSoundSaver',
           'spectrogram_u8', 'spectrogram_stack_u8', 'DeviceImageDataset', 'NearestNeighbours', 'NDB', 'NDBMonitor', 'LossMonitor', 'HealthMonitor', 'ScalarStats', 'SegmentStats',
           'TrainingDiverged', 'Sampler', 'sampler_for', 'Projector', 'ProjectionMonitor', 'project_samples', 'DeviceStripDataset', 'CropStream', 'spectrogram_strip_u8',
           'ChannelSlicedWasserstein', 'MelTable', 'mel_table', 'mel_analyse', 'mel_spectrum', 'mel_synthesise',
           'ResampleTable', 'resample_table', 'resample', 'resampled_length', 'load_wav', 'ShiftNearestNeighbours', 'ShiftNNMonitor',
           'PrecisionRecall', 'PRDMonitor', 'Augmenter', 'AugmentController', 'RandomEmbedding', 'FrechetDistance', 'frechet_statistic', 'FDMonitor',
           'KernelDistance', 'kid_statistic', 'KIDMonitor']
