"""CPU tier of the bf16 sampling path (pggan-pytorch_amd/sampling.py, include/pggan_hip_sampling.h): the test reference is the
reference network when nothing is rounded, its rounding function is torch's, the header parses into tables of its own, every consumer
validates ``precision`` and is unchanged by default, and the sampler names the layer it cannot take."""
import pytest
import torch

import sampling_ref as ref
from conftest import load_fixture
from helpers import build_flag_nets, build_nets, load_fixture_params

import pggan_amd as pg


def _golden_generators():
    for name in ('tiny32', 'tiny16c1'):
        yield name, None
    for case in load_fixture('flags16')[0]['cases']:                    # ReLU, no weight scaling, no PixelNorm / latent normalisation
        yield 'flags16', case['tag']


@pytest.mark.parametrize('name,tag', list(_golden_generators()))
def test_unrounded_reference_is_the_oracle_generator(oracle, name, tag):
    """generator_ref(rounded=False) against oracle.pggan_cpu.generator_forward in fp64 on the golden networks: the twin the GPU tests
    are held to is the same network."""
    meta, data = load_fixture(name)
    c = meta['cfg']
    flags = {}
    if tag is None:
        G, _ = build_nets(meta)
        load_fixture_params(G, data, 'G')
    else:
        case = [k for k in meta['cases'] if k['tag'] == tag][0]
        G, _ = build_flag_nets(meta, case)
        load_fixture_params(G, data, tag + '/G')
        g = case['g']
        flags = dict(normalize_latents=g.get('normalize_latents', True), wscale=g.get('wscale', True),
                     g_pixelnorm=g.get('pixelnorm', True), leakyrelu=g.get('leakyrelu', True))
    cfg = oracle.NetCfg(c['resolution'], c['num_channels'], fmap_base=c['fmap_base'], fmap_decay=c['fmap_decay'], fmap_max=c['fmap_max'],
                        latent_size=c['latent_size'], **flags)
    p64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in G.reference_state_dict().items()}
    z = torch.randn(3, c['latent_size'], dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    worst = 0.0
    for depth in range(G.max_depth + 1):
        for alpha in (1.0, 0.37):
            want = oracle.generator_forward(p64, cfg, z, depth, alpha)
            got = ref.generator_ref(G, z, rounded=False, depth=depth, alpha=alpha)
            assert got.shape == want.shape
            worst = max(worst, float((got - want).abs().max() / want.abs().max()))
    print('largest relative difference from the oracle: %.3e' % worst)
    assert worst <= 1e-12


def test_rne_is_torch_bfloat16_conversion():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-38, torch.randn(4096, generator=g) * 1e-41,
                   torch.randn(4096, generator=g) * 1e37, ref.special_values()])
    finite = x[~torch.isnan(x)]
    want = finite.to(torch.bfloat16)
    got = ref.rne_bf16(finite)
    assert torch.equal(ref.bf16_bits(got), ref.bf16_bits(want.float()))
    assert torch.equal(ref.bf16_bits(ref.rne_bf16(finite.double())), ref.bf16_bits(want.float()))     # (fp64 operands round the same way)
    assert bool(torch.isnan(ref.rne_bf16(torch.tensor([float('nan')]))).all())
    # half an ulp: the distance of the grid's midpoints
    one = torch.tensor([1.0, 1.5, 2.0, 3.0e-39], dtype=torch.float64)
    assert ref.half_ulp_bf16(one).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -134]


def test_header_parses_into_its_own_tables():
    sig, const = pg._lib.SAMPLING_SIGNATURES, pg._lib.SAMPLING_CONSTANTS
    assert set(sig) == {'pg_smp_cast_bf16', 'pg_smp_conv3_bf16', 'pg_smp_pixelnorm_bf16', 'pg_smp_torgb_bf16'}
    assert const['PG_SMP_UPSAMPLE'] == 1 and const['PG_SMP_PIXELNORM'] == 2 and const['PG_SMP_OUT_F32'] == 4
    others = (pg._lib.SIGNATURES, pg._lib.DEBUG_SIGNATURES, pg._lib.CLUSTER_SIGNATURES, pg._lib.GAN_SIGNATURES, pg._lib.PHASE_SIGNATURES)
    assert all(not set(sig) & set(o) for o in others)
    assert not set(const) & set(pg._lib.CONSTANTS)
    assert all(len(a) >= 4 for a in sig.values())                       # (the stream is the last of at least four arguments)
    assert pg.sampling.PIXELNORM_MAX_COUT == const['PG_SMP_PIXELNORM_MAX_COUT']


class _Trainer(object):
    parallel = None
    g_ema = None

    def __init__(self, G):
        self.G = G


def _small_generator():
    return pg.Generator((1, 3, 8, 8), fmap_base=32, fmap_max=16, latent_size=16)


def test_precision_is_validated_by_every_consumer(tmp_path):
    fn = lambda n: torch.zeros(n, 16)
    makers = {
        'OutputGenerator': lambda p: pg.OutputGenerator(fn, [], precision=p),
        'SWDMonitor': lambda p: pg.SWDMonitor(fn, fn, precision=p),
        'MSSSIMMonitor': lambda p: pg.MSSSIMMonitor(fn, precision=p),
        'NNMonitor': lambda p: pg.NNMonitor([], fn, precision=p),
        'NDBMonitor': lambda p: pg.NDBMonitor([], fn, precision=p),
        '_output_generator': lambda p: pg.plugins._output_generator(_Trainer(_small_generator()), None, precision=p),
        'output_samples': lambda p: pg.utils.output_samples(str(tmp_path / 'missing.dat'), 1, [], 'x', precision=p),
    }
    for name, make in makers.items():
        for bad in ('fp16', 'BF16', None, 16):
            with pytest.raises(ValueError, match='precision'):
                make(bad)
    for name in ('OutputGenerator', 'SWDMonitor', 'MSSSIMMonitor', 'NNMonitor', 'NDBMonitor'):
        assert makers[name]('bf16').precision == 'bf16'
        assert makers[name]('fp32').precision == 'fp32'
    assert pg.OutputGenerator(fn, []).precision == pg.SWDMonitor(fn, fn).precision == pg.MSSSIMMonitor(fn).precision == 'fp32'
    assert pg.NNMonitor([], fn).precision == pg.NDBMonitor([], fn).precision == 'fp32'


def test_default_output_generator_is_unchanged():
    G = _small_generator()
    tr = _Trainer(G)
    assert pg.plugins._output_generator(tr, None) is G
    assert pg.plugins._output_generator(tr, False, precision='fp32') is G
    s = pg.plugins._output_generator(tr, None, precision='bf16')
    assert isinstance(s, pg.Sampler) and s is pg.sampler_for(G) and s.network() is G
    assert callable(s.forward)


def test_sampler_sets_nothing_on_the_network_and_dies_with_it():
    import gc
    import weakref
    G = _small_generator()
    before = {id(m): set(vars(m)) for m in G.modules()}
    rt_before = set(G._rt.__slots__)
    s = pg.sampler_for(G)
    assert {id(m): set(vars(m)) for m in G.modules()} == before and set(G._rt.__slots__) == rt_before
    assert pg.sampler_for(G) is s
    w = weakref.ref(G)
    del G
    gc.collect()
    assert w() is None                                                  # the cache does not keep the network alive
    with pytest.raises(RuntimeError):
        s.network()


def test_sampler_refuses_a_12_channel_layer_by_name():
    G = pg.Generator((1, 3, 8, 8), fmap_base=48, fmap_max=16, latent_size=16)     # blocks.0: 16 -> 12 -> 12
    assert G.blocks[0].c1.ch_out == 12
    with pytest.raises(ValueError, match=r'blocks\.0\.c1.*16 -> 12'):
        pg.Sampler(G)
    with pytest.raises(ValueError, match='Generator'):
        pg.Sampler(torch.nn.Linear(2, 2))


def test_no_cpu_path():
    G = _small_generator()
    with pytest.raises(RuntimeError):
        pg.Sampler(G)(torch.zeros(2, 16))
