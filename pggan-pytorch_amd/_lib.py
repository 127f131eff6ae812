"""ctypes binding of libpggan_hip.so, derived at import from the C headers that declare its ABI.

include/pggan_hip.h (the product boundary), include/pggan_hip_debug.h (thread-local diagnostic exports) and
include/pggan_hip_cluster.h, include/pggan_hip_gan.h, include/pggan_hip_phase.h, include/pggan_hip_sampling.h,
include/pggan_hip_projection.h, include/pggan_hip_crop.h, include/pggan_hip_swd.h, include/pggan_hip_mel.h, include/pggan_hip_resample.h, include/pggan_hip_shift.h, include/pggan_hip_prd.h, include/pggan_hip_augment.h, include/pggan_hip_embed.h and include/pggan_hip_kid.h (the k-means, the GAN-objective, the magnitude +
instantaneous-frequency, the bf16 sampling, the projection-loss, the strip-crop, the C-channel sliced-Wasserstein, the warped-row sound, the rate-conversion, the shift-search, the k-NN-ball, the augmentation, the random-embedding and the kernel-distance additions to the boundary) are the one statement
of the ABI: the compiler holds every definition in csrc/*.hip against them, and this module parses them once into SIGNATURES /
DEBUG_SIGNATURES / CLUSTER_SIGNATURES / GAN_SIGNATURES / PHASE_SIGNATURES / SAMPLING_SIGNATURES / PROJECTION_SIGNATURES / CROP_SIGNATURES / SWD_SIGNATURES / MEL_SIGNATURES / RESAMPLE_SIGNATURES / SHIFT_SIGNATURES / PRD_SIGNATURES / AUGMENT_SIGNATURES / EMBED_SIGNATURES / KID_SIGNATURES (name -> argtypes), the
return types, and CONSTANTS / CLUSTER_CONSTANTS / GAN_CONSTANTS / PHASE_CONSTANTS / SAMPLING_CONSTANTS / PROJECTION_CONSTANTS / CROP_CONSTANTS / SWD_CONSTANTS / MEL_CONSTANTS / RESAMPLE_CONSTANTS / SHIFT_CONSTANTS / PRD_CONSTANTS / AUGMENT_CONSTANTS / EMBED_CONSTANTS / KID_CONSTANTS (every
``#define PG_*`` of the product header / of an addition as an integer).  A new entry point is
declared in the header, defined in csrc/ and wrapped in ops.py; nothing is restated here.

There is deliberately NO fallback: a prototype or ``#define`` the parser does not fully understand, a missing shared library or an
absent symbol fails loudly (``PgganLibraryError``).  Build the library with ``python __graft_entry__.py`` (or
``__graft_entry__.build()``)."""
import ast
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PGGAN_HIP_LIB') or os.path.join(_HERE, 'libpggan_hip.so')   # env override: kernel A/B experiments
_INCLUDE = os.path.join(os.path.dirname(_HERE), 'include')


class PgganLibraryError(RuntimeError):
    pass


P = ctypes.c_void_p
I = ctypes.c_int
L = ctypes.c_int64
F = ctypes.c_float
D = ctypes.c_double

_ARGTYPES = {'pg_stream_t': P, 'int': I, 'int64_t': L, 'float': F, 'double': D, 'size_t': ctypes.c_size_t, 'uint64_t': ctypes.c_uint64}
_RESTYPES = {'int': I, 'const char*': ctypes.c_char_p}


def _define_value(name, text):
    """Value of ``#define name text``: integer literals, parentheses, unary minus and <<; anything else is refused."""
    def value(node):
        if isinstance(node, ast.Constant) and type(node.value) is int:
            return node.value
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            return -value(node.operand)
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.LShift):
            return value(node.left) << value(node.right)
        raise PgganLibraryError('#define %s %s: not an integer expression' % (name, text))
    try:
        return value(ast.parse(text.strip(), mode='eval').body)
    except SyntaxError:
        raise PgganLibraryError('#define %s %s: not an integer expression' % (name, text))


def _argtype(name, param):
    if '*' in param:
        return P
    words = [w for w in param.split() if w != 'const']
    ctype = ' '.join(words[:-1])                    # the last word is the parameter's name
    if ctype not in _ARGTYPES or not re.fullmatch(r'[A-Za-z_]\w*', words[-1]):
        raise PgganLibraryError('%s: parameter "%s" has no ctypes mapping' % (name, ' '.join(param.split())))
    return _ARGTYPES[ctype]


def parse_header(text):
    """C header text -> (argtypes by name, restype by name, {PG_* define: int}) of its pg_* prototypes."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    guards = set(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]*$', text, flags=re.M))     # include guard: #ifndef X / #define X
    constants, body, conditionals = {}, [], []
    for line in text.split('\n'):
        directive = re.match(r'\s*#\s*(\w+)\s*(.*?)\s*$', line)
        foreign = next((c for c in conditionals if c), None)
        if foreign and re.search(r'\bpg_\w+\s*\(|#\s*define\s+PG_', line):
            raise PgganLibraryError('declaration under the preprocessor conditional "%s": %s' % (foreign, line.strip()))
        if not directive:
            body.append(line)
            continue
        word, rest = directive.groups()
        if word in ('if', 'ifdef', 'ifndef'):
            known = (word, rest) == ('ifdef', '__cplusplus') or word == 'ifndef' and rest in guards
            conditionals.append(None if known else line.strip())
        elif word == 'endif':
            conditionals.pop()
        elif word == 'define' and rest.startswith('PG_'):
            name, value = re.match(r'(\w+)(.*)', rest).groups()
            constants[name] = _define_value(name, value)
    body = '\n'.join(body)
    argtypes, restypes = {}, {}
    for m in re.finditer(r'\b(pg_\w+)\s*\(', body):
        name = m.group(1)
        params = re.compile(r'([^()]*)\)\s*;').match(body, m.end())
        if not params:
            raise PgganLibraryError('%s: cannot read the parameter list' % name)
        ret = ' '.join(body[max(body.rfind(c, 0, m.start()) for c in ';{}') + 1:m.start()].split()).replace(' *', '*')
        if ret not in _RESTYPES:
            raise PgganLibraryError('%s: return type "%s" has no ctypes mapping' % (name, ret))
        params = [p.strip() for p in params.group(1).split(',')]
        argtypes[name] = [] if params in ([''], ['void']) else [_argtype(name, p) for p in params]
        restypes[name] = _RESTYPES[ret]
    return argtypes, restypes, constants


def _read_header(name):
    try:
        with open(os.path.join(_INCLUDE, name)) as f:
            return parse_header(f.read())
    except OSError as e:
        raise PgganLibraryError('cannot read the C-ABI header %s: %s' % (name, e))


# name -> argtypes (stream is always the last void*) of the product boundary, of the diagnostic exports; name -> restype of both
SIGNATURES, _RESTYPE_OF, CONSTANTS = _read_header('pggan_hip.h')
DEBUG_SIGNATURES, _debug_restypes, _ = _read_header('pggan_hip_debug.h')
_RESTYPE_OF.update(_debug_restypes)
# an addition to the product boundary with tables of its own (k-means bins of NDB/k: csrc/cluster.hip, wrapped in cluster.py)
CLUSTER_SIGNATURES, _cluster_restypes, CLUSTER_CONSTANTS = _read_header('pggan_hip_cluster.h')
_RESTYPE_OF.update(_cluster_restypes)
# ... and the loss block of the selectable GAN objectives (csrc/gan_losses.hip, wrapped in ops.py, public through gan_losses.py)
GAN_SIGNATURES, _gan_restypes, GAN_CONSTANTS = _read_header('pggan_hip_gan.h')
_RESTYPE_OF.update(_gan_restypes)
# ... and the magnitude + instantaneous-frequency sound ends with the two-channel real batch (csrc/phase.hip, wrapped in phase.py)
PHASE_SIGNATURES, _phase_restypes, PHASE_CONSTANTS = _read_header('pggan_hip_phase.h')
_RESTYPE_OF.update(_phase_restypes)
# ... and the forward-only bf16 generator of the samplers and metric monitors (csrc/sampling.hip, wrapped in sampling.py)
SAMPLING_SIGNATURES, _sampling_restypes, SAMPLING_CONSTANTS = _read_header('pggan_hip_sampling.h')
_RESTYPE_OF.update(_sampling_restypes)
# ... and the pyramid loss of the latent projection with its image gradient (csrc/projection.hip, wrapped in ops.py, used by projection.py)
PROJECTION_SIGNATURES, _projection_restypes, PROJECTION_CONSTANTS = _read_header('pggan_hip_projection.h')
_RESTYPE_OF.update(_projection_restypes)
# ... and the real batch cut from spectrogram strips at random time offsets (csrc/real_batch.hip: the batch kernels' strip source; wrapped in ops.py, used by dataset.py)
CROP_SIGNATURES, _crop_restypes, CROP_CONSTANTS = _read_header('pggan_hip_crop.h')
_RESTYPE_OF.update(_crop_restypes)
# ... and the descriptor side of the sliced Wasserstein distance for 1 .. 4 channels (csrc/swd.hip, wrapped in ops.py, used by metrics.py)
SWD_SIGNATURES, _swd_restypes, SWD_CONSTANTS = _read_header('pggan_hip_swd.h')
_RESTYPE_OF.update(_swd_restypes)
# ... and the magnitude + instantaneous-frequency sound ends on warped (mel) rows (csrc/mel.hip, wrapped in phase.py)
MEL_SIGNATURES, _mel_restypes, MEL_CONSTANTS = _read_header('pggan_hip_mel.h')
_RESTYPE_OF.update(_mel_restypes)
# ... and the polyphase rate conversion in front of the sound ends (csrc/resample.hip, wrapped in sound.py)
RESAMPLE_SIGNATURES, _resample_restypes, RESAMPLE_CONSTANTS = _read_header('pggan_hip_resample.h')
_RESTYPE_OF.update(_resample_restypes)
# ... and the nearest windows at every start column of the strips (csrc/shift_search.hip, wrapped in ops.py, used by metrics.py)
SHIFT_SIGNATURES, _shift_restypes, SHIFT_CONSTANTS = _read_header('pggan_hip_shift.h')
_RESTYPE_OF.update(_shift_restypes)
# ... and the tile kernel of precision / recall / density / coverage over k-NN balls (csrc/prd.hip, wrapped in ops.py, used by metrics.py)
PRD_SIGNATURES, _prd_restypes, PRD_CONSTANTS = _read_header('pggan_hip_prd.h')
_RESTYPE_OF.update(_prd_restypes)
# ... and the differentiable augmentation of D's inputs: gather, transpose, parameter table, sign count (csrc/augment.hip, wrapped in ops.py, used by augment.py)
AUGMENT_SIGNATURES, _augment_restypes, AUGMENT_CONSTANTS = _read_header('pggan_hip_augment.h')
_RESTYPE_OF.update(_augment_restypes)
# ... and the ends of the random convolutional embedding with the fp64 moments of its features (csrc/embed.hip, wrapped in ops.py, used by metrics.py)
EMBED_SIGNATURES, _embed_restypes, EMBED_CONSTANTS = _read_header('pggan_hip_embed.h')
_RESTYPE_OF.update(_embed_restypes)
# ... and the tile sums of the cubic polynomial kernel for the unbiased kernel distance (csrc/kid.hip, wrapped in ops.py, used by metrics.py)
KID_SIGNATURES, _kid_restypes, KID_CONSTANTS = _read_header('pggan_hip_kid.h')
_RESTYPE_OF.update(_kid_restypes)
ABI_VERSION = CONSTANTS['PG_ABI_VERSION']          # load() holds the library's pg_abi_version() against it: a stale .so is refused

_lib = None


def load():
    """Load the shared library once and declare every prototype.  Raises PgganLibraryError."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PgganLibraryError(
            'libpggan_hip.so not found at %s: the HIP extension is not built (run '
            '`python __graft_entry__.py`). There is no CPU fallback.' % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise PgganLibraryError('cannot load %s: %s' % (LIB_PATH, e))
    for name, argtypes in (list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()) + list(CLUSTER_SIGNATURES.items())
                           + list(GAN_SIGNATURES.items()) + list(PHASE_SIGNATURES.items()) + list(SAMPLING_SIGNATURES.items())
                           + list(PROJECTION_SIGNATURES.items()) + list(CROP_SIGNATURES.items()) + list(SWD_SIGNATURES.items())
                           + list(MEL_SIGNATURES.items()) + list(RESAMPLE_SIGNATURES.items()) + list(SHIFT_SIGNATURES.items())
                           + list(PRD_SIGNATURES.items()) + list(AUGMENT_SIGNATURES.items()) + list(EMBED_SIGNATURES.items())
                           + list(KID_SIGNATURES.items())):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise PgganLibraryError('symbol %s missing from %s' % (name, LIB_PATH))
        fn.argtypes = argtypes
        fn.restype = _RESTYPE_OF[name]
    v = lib.pg_abi_version()
    if v != ABI_VERSION:
        raise PgganLibraryError('ABI version mismatch: library %d, binding %d' % (v, ABI_VERSION))
    _lib = lib
    return lib


_ERR = {CONSTANTS['PG_E_ARG']: 'PG_E_ARG (bad dimension / null pointer)', CONSTANTS['PG_E_ALIGN']: 'PG_E_ALIGN (channel count / alignment)',
        CONSTANTS['PG_E_UNSUP']: 'PG_E_UNSUP (unsupported configuration)', CONSTANTS['PG_E_NOLIB']: 'PG_E_NOLIB (no RCCL library could be loaded)'}
_E_UNSUP, _E_RCCL_BASE = CONSTANTS['PG_E_UNSUP'], CONSTANTS['PG_E_RCCL_BASE']


class Unsupported(RuntimeError):
    """PG_E_UNSUP: the entry point does not take this configuration (callers with a fallback catch exactly this)."""


def check(rc, name):
    if rc != 0:
        what = _ERR.get(rc) or ('RCCL ncclResult_t %d' % (_E_RCCL_BASE - rc) if rc <= _E_RCCL_BASE else 'hipError_t %d' % rc)
        raise (Unsupported if rc == _E_UNSUP else RuntimeError)('%s failed: %s' % (name, what))


CALL_HOOK = None        # measurement aid (bench.py): ``hook(fn, args, name) -> rc`` runs every C-ABI call, eager or replayed from a launch plan


def call(name, *args):
    """Invoke a C-ABI entry point and raise on a non-zero return."""
    fn = getattr(load(), name)
    check(fn(*args) if CALL_HOOK is None else CALL_HOOK(fn, args, name), name)
