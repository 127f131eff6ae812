"""The ctypes binding is derived from the C headers (pggan-pytorch_amd/_lib.py): the parser on small synthetic headers, what it
refuses, and the real include/*.h held against an independent regex.  Host tests: no GPU, no shared library."""
import ctypes
import os
import re

import pytest

import pggan_amd as pg

_lib = pg._lib
P, I, L, F, D = _lib.P, _lib.I, _lib.L, _lib.F, _lib.D
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


SYNTHETIC = """
/* A comment with a prototype in it: int pg_not_this(int a, float b); and stray ( , ; characters */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PG_E_RCCL_BASE (-16) /* (not, this; one) */
#define PG_BIG (1 << 22)     // nor ( this , one ;
#define PG_PLAIN 147
typedef void* pg_stream_t;
enum pg_kind { PG_KIND_A = 0, PG_KIND_B = 1 };
// int pg_nor_this(void);
int pg_multi(const float* x, /* host ( */ const unsigned char* bytes,
             const int64_t* off,   // , ; (
             void* p, int n, int64_t m,
             float a, double b, size_t s, uint64_t seed,
             const int flag, pg_stream_t stream);
int pg_none(void);
int pg_empty();
const char* pg_name(void);
const char *pg_name2(int which);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_a_synthetic_header():
    args, res, consts = _lib.parse_header(SYNTHETIC)
    assert list(args) == ['pg_multi', 'pg_none', 'pg_empty', 'pg_name', 'pg_name2']          # nothing from the comments
    got = args['pg_multi']
    want = [P, P, P, P, I, L, F, D, ctypes.c_size_t, ctypes.c_uint64, I, P]
    assert len(got) == len(want) and all(g is w for g, w in zip(got, want)), got
    assert args['pg_none'] == [] and args['pg_empty'] == [] and args['pg_name'] == [] and args['pg_name2'] == [I]
    assert res == {'pg_multi': I, 'pg_none': I, 'pg_empty': I, 'pg_name': ctypes.c_char_p, 'pg_name2': ctypes.c_char_p}
    assert consts == {'PG_E_RCCL_BASE': -16, 'PG_BIG': 1 << 22, 'PG_PLAIN': 147}
    assert all(type(v) is int for v in consts.values())


@pytest.mark.parametrize('header, named', [
    ('int pg_f(long n);', 'long'),
    ('int pg_f(int a, unsigned n);', 'unsigned'),
    ('int pg_f(short n, int b);', 'short'),
    ('int pg_f(struct pg_dims d);', 'struct pg_dims'),
    ('int pg_f(int);', 'int'),                                     # unnamed: the last word would be taken for the name
    ('int pg_f(int n[4]);', 'n[4]'),                               # an array parameter is a pointer in C, an int to the type map
    ('int pg_f(int n, ...);', '...'),
    ('void pg_f(int n);', 'void'),
    ('float pg_f(int n);', 'float'),
    ('int64_t pg_f(int n);', 'int64_t'),
    ('static inline int pg_f(int n);', 'static inline int'),
    ('int pg_f(int (*callback)(int), int n);', 'pg_f'),            # half-matched: the parameter list does not close
    ('int pg_f(int n) { return n; }', 'pg_f'),                     # a definition, not a prototype
    ('int pg_f(int n', 'pg_f'),
    ('#define PG_X 1.5', 'PG_X'),
    ('#define PG_X', 'PG_X'),
    ('#define PG_X (1 + 2)', 'PG_X'),
    ('#define PG_X PG_Y', 'PG_X'),
    ('#define PG_X(a) 1', 'PG_X'),
    ('#define PG_X __import__("os").getpid()', 'PG_X'),
    ('#define PG_X 1 << 2 \\\n  << 3', 'PG_X'),
    ('#ifdef SOMETHING\nint pg_f(int n);\n#endif', 'SOMETHING'),
    ('#if defined(__cplusplus)\nint pg_f(int n);\n#endif', '__cplusplus'),
    ('#ifndef NOT_A_GUARD\nint pg_f(\n  int n);\n#endif', 'NOT_A_GUARD'),
    ('#ifdef SOMETHING\n#define PG_X 1\n#endif', 'SOMETHING'),
    ('#ifdef __cplusplus\n#ifdef SOMETHING\nint pg_f(int n);\n#endif\n#endif', 'SOMETHING'),
])
def test_parser_refuses_what_it_does_not_understand(header, named):
    with pytest.raises(_lib.PgganLibraryError) as e:
        _lib.parse_header(header)
    assert named in str(e.value), str(e.value)


def test_conditionals_close():
    """A prototype after the #endif of a foreign conditional is outside it again; #ifdef __cplusplus and the guard never count."""
    args, _, consts = _lib.parse_header('#ifndef G_H\n#define G_H\n#ifdef SOMETHING\ntypedef int t;\n#else\n#endif\n'
                                        '#ifdef __cplusplus\nextern "C" {\n#endif\nint pg_f(int n);\n#define PG_X -3\n#endif\n')
    assert args == {'pg_f': [I]} and consts == {'PG_X': -3}


def test_real_headers_are_derived_completely():
    """Every prototype that the independent regex of test_library_exports_every_declared_symbol finds is in the derived tables and
    nothing else is; CONSTANTS holds every #define PG_* of the product header."""
    proto = r'\b(?:int|const char\*)\s+(pg_\w+)\s*\('
    hdr, dbg = _read('include', 'pggan_hip.h'), _read('include', 'pggan_hip_debug.h')
    assert set(re.findall(proto, hdr)) == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 96
    assert set(re.findall(proto, dbg)) == set(_lib.DEBUG_SIGNATURES) and len(_lib.DEBUG_SIGNATURES) == 7
    chars = {n for n in _lib.DEBUG_SIGNATURES if n.startswith('pg_debug_last_')}
    assert len(chars) == 3
    _, res, _ = _lib.parse_header(hdr)
    _, res_dbg, dbg_consts = _lib.parse_header(dbg)
    assert all(r is I for r in res.values()) and len(res) == 96
    assert {n for n, r in res_dbg.items() if r is ctypes.c_char_p} == chars and all(res_dbg[n] is I for n in set(res_dbg) - chars)
    assert dbg_consts == {}                                       # its enums need no Python mirror
    defines = dict(re.findall(r'^#define[ \t]+(PG_\w+)[ \t]+(\S.*?)[ \t]*(?:/\*.*)?$', hdr, flags=re.M))
    assert set(defines) == set(_lib.CONSTANTS) and len(_lib.CONSTANTS) == 27 and 'PG_ABI_VERSION' in defines
    for name, text in defines.items():
        assert re.fullmatch(r'[-\d()< ]+', text), (name, text)
        assert _lib.CONSTANTS[name] == eval(text), name           # the text is digits, parentheses, '-' and '<<' only
    assert _lib.ABI_VERSION == _lib.CONSTANTS['PG_ABI_VERSION'] == 27
    assert 'return PG_ABI_VERSION;' in _read('pggan-pytorch_amd', 'csrc', 'elementwise.hip')


# Python name -> the header's name, for every constant of ops.py that mirrors a #define
OPS_MIRRORS = {
    'FLAG_UPSAMPLE': 'PG_FLAG_UPSAMPLE', 'FLAG_MASK_BYTES': 'PG_FLAG_MASK_BYTES', 'FLAG_Y_BYTES': 'PG_FLAG_Y_BYTES',
    'FLAG_SIGNS_OUT': 'PG_FLAG_SIGNS_OUT', 'MBSTD_STATS_STRIDE': 'PG_MBSTD_STATS_STRIDE', 'SWD_DESC': 'PG_SWD_DESC',
    'SWD_REDUCE_BLOCKS': 'PG_SWD_REDUCE_BLOCKS', 'SWD_SORT_LDS_ROW': 'PG_SWD_SORT_RUN', 'SWD_SORT_MERGE_RUN': 'PG_SWD_SORT_RUN',
    'SWD_SORT_MERGE_TILE': 'PG_SWD_SORT_MERGE_TILE', 'SWD_SORT_MAX_M': 'PG_SWD_SORT_MAX_M', 'MSSSIM_TILE': 'PG_MSSSIM_TILE',
    'NN_MAX_QUERIES': 'PG_NN_MAX_QUERIES', 'NN_MAX_TOPK': 'PG_NN_MAX_TOPK', 'STATS_MAX_SOURCES': 'PG_STATS_MAX_SOURCES',
    'STATS_RECORD': 'PG_STATS_RECORD', 'STATS_MAX_LENGTH': 'PG_STATS_MAX_LENGTH', 'SEG_CHUNK': 'PG_SEG_CHUNK',
}


def test_no_constant_is_restated():
    """Every PG_* name that ops.py, parallel.py and _lib.py use is a key of CONSTANTS, the module attribute made from it has the
    header's value, and no number stands beside a comment that names a define."""
    C = _lib.CONSTANTS
    for name, define in OPS_MIRRORS.items():
        assert getattr(pg.ops, name) == C[define] and type(getattr(pg.ops, name)) is int, name
    assert pg.ops.SOUND_MODES == {'abslog': C['PG_SOUND_ABSLOG'], 'reallog': C['PG_SOUND_REALLOG']}
    assert len(pg.ops.MSSSIM_WEIGHTS) == C['PG_MSSSIM_MAX_SCALES']
    assert set(_lib._ERR) == {C['PG_E_ARG'], C['PG_E_ALIGN'], C['PG_E_UNSUP'], C['PG_E_NOLIB']}
    for define in ('PG_E_ARG', 'PG_E_ALIGN', 'PG_E_UNSUP', 'PG_E_NOLIB'):
        assert _lib._ERR[C[define]].startswith(define + ' ')
    with pytest.raises(pg.ops.Unsupported):
        _lib.check(C['PG_E_UNSUP'], 'f')
    with pytest.raises(RuntimeError, match=r'ncclResult_t 2\b'):
        _lib.check(C['PG_E_RCCL_BASE'] - 2, 'f')
    with pytest.raises(RuntimeError, match=r'hipError_t 700\b'):
        _lib.check(700, 'f')
    for module in ('ops.py', 'parallel.py', '_lib.py'):
        src = _read('pggan-pytorch_amd', module)
        keys = set(re.findall(r"""\[['"](PG_\w+)['"]\]""", src))
        assert keys <= set(C), keys - set(C)
        for line in src.split('\n'):                              # "X = 136   # PG_X of include/..." is what this replaced
            assert not re.match(r'[^#]*=\s*[-(\d][^#\[]*#.*\bPG_[A-Z]', line), line
    assert set(OPS_MIRRORS.values()) | {'PG_SOUND_ABSLOG', 'PG_SOUND_REALLOG', 'PG_MSSSIM_MAX_SCALES'} == \
        set(re.findall(r"_C\['(PG_\w+)'\]", _read('pggan-pytorch_amd', 'ops.py')))
    par = _read('pggan-pytorch_amd', 'parallel.py')
    assert par.count("create_string_buffer(") == 2 and '128' not in par and "CONSTANTS['PG_COMM_ID_BYTES']" in par
