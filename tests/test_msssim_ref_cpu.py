"""tests/msssim_ref.py, the CPU statement of the MS-SSIM definition, pinned on its own: the device tests
(tests/test_msssim_gpu.py) hold the kernels against it, so it has to be right first."""
import numpy as np
import pytest
import torch

import msssim_ref as ref


def _noise_pairs():
    """Independent uniform noise at 16x16, one channel, 8 pairs (seed 0): the case with negative mean terms."""
    g = torch.Generator().manual_seed(0)
    a = torch.rand(8, 1, 16, 16, generator=g, dtype=torch.float32) * 2 - 1
    b = torch.rand(8, 1, 16, 16, generator=g, dtype=torch.float32) * 2 - 1
    return a, b


def test_single_scale_maps_agree_with_scipy():
    signal = pytest.importorskip('scipy.signal')
    rs = np.random.RandomState(3)
    a, b = rs.rand(2, 3, 32, 32) * 255, rs.rand(2, 3, 32, 32) * 255
    g = np.array([np.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)])
    g /= g.sum()
    win = np.outer(g, g)                                                   # built here, not taken from the reference

    def filt(x):
        return signal.convolve2d(x, win[::-1, ::-1], mode='valid')

    ssim, cs = ref.ssim_maps(torch.from_numpy(a), torch.from_numpy(b))
    assert tuple(ssim.shape) == (2, 3, 22, 22)
    for i in range(2):
        for c in range(3):
            x, y = a[i, c], b[i, c]
            mx, my = filt(x), filt(y)
            sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
            want_cs = (2 * sxy + (0.03 * 255) ** 2) / (sxx + syy + (0.03 * 255) ** 2)
            want = (2 * mx * my + (0.01 * 255) ** 2) / (mx * mx + my * my + (0.01 * 255) ** 2) * want_cs
            assert np.abs(cs[i, c].numpy() - want_cs).max() < 1e-12
            assert np.abs(ssim[i, c].numpy() - want).max() < 1e-12


def test_scales_and_weights():
    for r, count in ((16, 1), (32, 2), (64, 3), (128, 4), (256, 5), (512, 5), (1024, 5)):
        sides, weights = ref.scales(r)
        assert sides == [r >> s for s in range(count)] and min(sides) >= 16
        assert abs(sum(weights) - 1.0) < 1e-15
    assert ref.scales(256)[1] == pytest.approx([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], abs=1e-4)   # (the published five sum to 1.0001)
    assert abs(float(ref.taps(torch.float64).sum()) - 1.0) < 1e-15


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_identical_pair_is_exactly_one(dtype):
    g = torch.Generator().manual_seed(1)
    for shape in ((2, 1, 16, 16), (2, 3, 64, 64)):
        a = torch.rand(shape, generator=g, dtype=dtype) * 2 - 1
        values, terms = ref.msssim_pairs(a, a.clone())
        assert values.dtype == dtype and torch.all(values == 1.0) and torch.all(terms == 1.0)


def test_symmetric_and_pairs_are_independent():
    g = torch.Generator().manual_seed(2)
    a = torch.rand(3, 3, 32, 32, generator=g, dtype=torch.float64) * 2 - 1
    b = (a + 0.3 * torch.randn(3, 3, 32, 32, generator=g, dtype=torch.float64)).clamp(-1, 1)
    v_ab, t_ab = ref.msssim_pairs(a, b)
    v_ba, t_ba = ref.msssim_pairs(b, a)
    assert torch.allclose(v_ab, v_ba, rtol=0, atol=1e-14) and torch.allclose(t_ab, t_ba, rtol=0, atol=1e-14)
    assert float(v_ab.min()) > 0.0 and float(v_ab.max()) < 1.0
    # b = a with one image replaced: the other pairs stay at their value
    b2 = a.clone()
    b2[1] = b[1]
    v2, _ = ref.msssim_pairs(a, b2)
    assert v2[0] == 1.0 and v2[2] == 1.0 and v2[1] == v_ab[1]


def test_quantisation_levels():
    # drange (-255, 255) makes the scale 0.5, so that x = 2 m + 1 - 255 lands exactly on the boundary m + 0.5
    x = torch.tensor([-300.0, -255.0, -254.0, -252.0, -250.0, 0.0, 253.0, 254.0, 255.0, 400.0], dtype=torch.float32)
    q = ref.quantise(x, drange=(-255, 255))
    assert q.tolist() == [0.0, 0.0, 0.0, 2.0, 2.0, 128.0, 254.0, 254.0, 255.0, 255.0]     # halves go to the even level: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 127.5 -> 128, 254.5 -> 254
    raw = ref.quantise(x, drange=(-255, 255), quantize=False)
    assert raw[0] == -22.5 and raw[-1] == 327.5 and raw[3] == 1.5
    y = torch.tensor([-1.5, -1.0, 0.0, 1.0, 2.0], dtype=torch.float32)
    assert ref.quantise(y).tolist() == [0.0, 0.0, 128.0, 255.0, 255.0]
    assert torch.equal(ref.pool(torch.tensor([[1.0, 2.0], [3.0, 5.0]]).view(1, 1, 2, 2)), torch.tensor([[[[2.75]]]]))


def test_unrelated_noise_has_a_negative_term_and_gives_zero():
    a, b = _noise_pairs()
    for dtype in (torch.float32, torch.float64):
        values, terms = ref.msssim_pairs(a.to(dtype), b.to(dtype))
        negative = terms[:, 0] < 0
        assert int(negative.sum()) >= 1
        assert torch.all(torch.isfinite(values)) and torch.all(values[negative] == 0.0) and torch.all(values[~negative] > 0.0)
    mean, std = ref.summary(values)
    assert 0.0 < mean < 0.1 and std > 0.0
