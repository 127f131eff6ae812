"""pg_resample_mono (include/pggan_hip_resample.h) between guard bands (tests/redzone.py, docs/experiments_redzone.md), patterned on
tests/test_melif_redzone_gpu.py: the four shapes whose signal is shorter than the filter -- every output has both edges of the
signal inside its taps -- and 3000 samples at 44100 -> 16000 (160 phases, five workgroups, a ragged last run), mono and stereo,
float32 and int16.  The signal and the table lie between bands (NaN for float data: an outside load that reaches a sum poisons it and
the comparison with the twin fails; int16 bands read as 32639), the output is filled with the sentinel: no byte outside a tensor is
read as data or written, every output byte is written, and the result equals tests/resample_ref.py with ``==``."""
import numpy as np
import pytest
import torch

import resample_ref as ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
sound, _lib, ops = pg.sound, pg._lib, pg.ops

SHAPES = [(3, 2, 1), (3, 2, 5), (2, 3, 7), (5, 7, 33), (44100, 16000, 3000)]


@pytest.fixture
def rz():
    r = Redzone('cuda')
    yield r
    r.forget()


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


@pytest.mark.parametrize('rate_in,rate_out,nsamp', SHAPES)
@pytest.mark.parametrize('channels', [1, 2])
def test_resample_inside_guard_bands(rz, rate_in, rate_out, nsamp, channels):
    L, M = ref.ratio(rate_in, rate_out)
    table = sound.resample_table(rate_in, rate_out)
    taps_d = rz.guard(torch.from_numpy(np.array(table.taps)), name='taps')
    n_out = ref.length(nsamp, rate_in, rate_out)
    RC = _lib.RESAMPLE_CONSTANTS
    for dtype, fmt in ((np.float32, RC['PG_RESAMPLE_F32']), (np.int16, RC['PG_RESAMPLE_I16'])):
        x = ref.signal(nsamp, 100 + nsamp + channels, channels, dtype)
        want = ref.vectorised(ref.mix(x), table.taps, L, M)
        x_d = rz.guard(torch.from_numpy(x), name='x.%s' % np.dtype(dtype).name)
        out = rz.out((n_out,), torch.float32, name='out')
        assert x_d.data_ptr() % 32 == 16 and taps_d.data_ptr() % 32 == 16 and out.data_ptr() % 32 == 16
        _lib.call('pg_resample_mono', x_d.data_ptr(), fmt, nsamp, channels, taps_d.data_ptr(), L, M, table.T, out.data_ptr(), n_out,
                  ops._stream())
        chk(rz)                                                # bands intact, the inputs unchanged, every output element written
        assert np.array_equal(out.cpu().numpy(), want)
        # the public function on the guarded signal, with the guarded table as its device copy
        guarded = sound.ResampleTable(L, M, table.taps)
        guarded._on[torch.device('cuda', torch.cuda.current_device())] = taps_d
        assert np.array_equal(sound.resample(x_d, rate_in, rate_out, table=guarded).cpu().numpy(), want)
        chk(rz)
