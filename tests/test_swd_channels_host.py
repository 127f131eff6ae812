"""Host side of the sliced Wasserstein distance for 1 .. 4 channels (include/pggan_hip_swd.h, metrics.ChannelSlicedWasserstein): the
binding of the new header, the constructor's argument checks (all of them come before the device is asked for) and the random draws.
No GPU."""
import ctypes
import os
import re

import pytest
import torch

import pggan_amd as pg

_lib = pg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['pg_swd_gather_c', 'pg_swd_channel_stats_c', 'pg_swd_normalize_c', 'pg_swd_project_c']


def test_swd_header_is_derived_completely_and_the_product_tables_are_unchanged():
    with open(os.path.join(ROOT, 'include', 'pggan_hip_swd.h')) as f:
        hdr = f.read()
    args, res, consts = _lib.parse_header(hdr)
    declared = re.findall(r'\b(?:int|const char\*)\s+(pg_\w+)\s*\(', hdr)                # (independent of the binding's parser)
    assert sorted(declared) == sorted(args) == sorted(_lib.SWD_SIGNATURES) == sorted(NAMES)
    P, I, L = _lib.P, _lib.I, _lib.L
    assert _lib.SWD_SIGNATURES == {'pg_swd_gather_c': [P, P, P, L, I, I, I, L, L, P], 'pg_swd_channel_stats_c': [P, L, I, P, P, P],
                                   'pg_swd_normalize_c': [P, L, I, P, P], 'pg_swd_project_c': [P, P, P, L, I, I, P]}
    assert all(r is I for r in res.values())
    defines = dict(re.findall(r'^#define[ \t]+(PG_\w+)[ \t]+(\d+)[ \t]*$', hdr, flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == consts == _lib.SWD_CONSTANTS == {'PG_SWD_PATCH': 49, 'PG_SWD_MAX_CHANNELS': 4}
    assert pg.ops.SWD_PATCH == 49 and pg.ops.SWD_MAX_CHANNELS == 4 and pg.ops.SWD_DESC == 3 * pg.ops.SWD_PATCH
    # additive: the product boundary is what it was
    assert len(_lib.SIGNATURES) == 96 and len(_lib.CONSTANTS) == 27 and _lib.ABI_VERSION == 27
    others = (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.CLUSTER_SIGNATURES, _lib.GAN_SIGNATURES, _lib.PHASE_SIGNATURES,
              _lib.SAMPLING_SIGNATURES, _lib.PROJECTION_SIGNATURES, _lib.CROP_SIGNATURES)
    assert not any(set(_lib.SWD_SIGNATURES) & set(o) for o in others)
    assert not set(_lib.SWD_CONSTANTS) & set(_lib.CONSTANTS)


def test_every_swd_prototype_is_registered_for_loading():
    """load() declares argtypes and restype of every name of the header on the library, and the library exports them."""
    assert all(_lib._RESTYPE_OF[name] is _lib.I for name in NAMES)
    if not os.path.exists(pg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(pg.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SWD_SIGNATURES[name] and fn.restype is _lib.I, name


def test_channel_count_of_a_width():
    assert [pg.ops.swd_channels(w) for w in (49, 98, 147, 196)] == [1, 2, 3, 4]
    for bad in (0, 48, 50, 7, 245, -49):
        with pytest.raises(ValueError):
            pg.ops.swd_channels(bad)


def test_constructor_argument_errors():
    CSW = pg.metrics.ChannelSlicedWasserstein
    assert pg.ChannelSlicedWasserstein is CSW and 'ChannelSlicedWasserstein' in pg.__all__
    assert issubclass(pg.metrics.SlicedWasserstein, CSW)
    for bad in (0, 5, -1, 2.5):
        with pytest.raises(ValueError, match='num_channels'):
            CSW(32, 4, bad)
    for bad in (8, 24, 0):
        with pytest.raises(ValueError, match='resolution'):
            CSW(bad, 4, 1)
    with pytest.raises(ValueError, match='resolution'):
        CSW(8, 4, 5)                                                       # the resolution is looked at first, as in SlicedWasserstein
    for kw in (dict(patches_per_image=0), dict(dir_repeats=0), dict(dirs_per_repeat=-1)):
        with pytest.raises(ValueError):
            CSW(32, 4, 2, **kw)
    with pytest.raises(ValueError):
        CSW(32, 0, 2)
    for C in (1, 2, 4):
        with pytest.raises(ValueError, match='descriptors'):
            CSW(128, 1 << 16, C, patches_per_image=128)                    # 2^23 descriptors: above SWD_SORT_MAX_M
    assert (1 << 16) * 128 > pg.ops.SWD_SORT_MAX_M
    # SlicedWasserstein keeps its contract and its message
    with pytest.raises(ValueError, match='3x7x7'):
        pg.metrics.SlicedWasserstein(32, 4, num_channels=1)
    with pytest.raises(ValueError, match='resolution'):
        pg.metrics.SlicedWasserstein(8, 4, num_channels=1)


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_directions_shape_and_unit_norm(C):
    levels, rows = pg.metrics.swd_levels(64), 5 * 8
    centres, dirs = pg.metrics.swd_draws(levels, rows, 4, 49 * C, 64, seed=1)
    assert tuple(dirs.shape) == (4, 49 * C, 64) and dirs.dtype == torch.float32 and dirs.is_contiguous()
    assert float((dirs.double().pow(2).sum(dim=1) - 1).abs().max()) < 1e-6
    assert len(centres) == 3
    for c, s in zip(centres, levels):
        assert tuple(c.shape) == (rows, 2) and c.dtype == torch.int32 and int(c.min()) >= 3 and int(c.max()) <= s - 4
    # the centres come first from the one generator, so they do not depend on C; the directions of C = 3 are the ones SlicedWasserstein
    # has always drawn: randint per level, then one randn [R, 147, K]
    c3, d3 = pg.metrics.swd_draws(levels, rows, 4, 147, 64, seed=1)
    assert all(torch.equal(a, b) for a, b in zip(centres, c3))
    gen = torch.Generator().manual_seed(1)
    want = [torch.randint(3, s - 3, (rows, 2), generator=gen, dtype=torch.int32) for s in levels]
    d = torch.randn(4, 147, 64, generator=gen, dtype=torch.float32).double()
    assert all(torch.equal(a, b) for a, b in zip(c3, want))
    assert torch.equal(d3, (d / d.pow(2).sum(dim=1, keepdim=True).sqrt()).float())
    other, _ = pg.metrics.swd_draws(levels, rows, 4, 49 * C, 64, seed=2)
    assert not torch.equal(other[0], centres[0])
