"""ctypes binding of ``libbrever_ffnn_stream.so`` (C ABI ``brv_ffs_*``, ``include/brever_ffnn_stream.h``,
kernels under ``csrc/ffnn_stream/``): the streaming kernels of the FFNN mask estimator. A library of its own next
to ``libbrever_hip.so``, bound the way ``mixture.py`` binds the mixture engine: the table is read from the
header, ``call`` / ``query`` raise with the library's own message. The streamer built on it is
``brever_amd.streaming.FFNNStreamer``. There is no CPU fallback.
"""
import ctypes
import os

from . import hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BRV_FFS_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libbrever_ffnn_stream.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'brever_ffnn_stream.h')

MAX_HIDDEN = 8           # BRV_FFS_MAX_HIDDEN
MAX_FEATURES = 6         # BRV_FFS_MAX_FEATURES


class FfsConfig(ctypes.Structure):
    """``brv_ffs_config`` -- geometry of an FFNN and the addresses its values live at."""
    _L = MAX_HIDDEN + 1
    _fields_ = [(name, ctypes.c_int32) for name in (
        'n_fft', 'frame_length', 'hop', 'channels', 'center', 'pad_constant', 'normalized', 'onesided')] + [
        ('compression', ctypes.c_float), ('scale', ctypes.c_float)] + [
        (name, ctypes.c_int32) for name in ('mel', 'stacks', 'features', 'norm')] + [
        ('feat_norm', ctypes.c_int32*MAX_FEATURES), ('feat_comp', ctypes.c_int32*MAX_FEATURES),
        ('eps_feat', ctypes.c_float), ('eps_norm', ctypes.c_float),
        ('hidden', ctypes.c_int32), ('reserved', ctypes.c_int32),
        ('widths', ctypes.c_int32*_L), ('reserved2', ctypes.c_int32),
        ('weight', ctypes.c_void_p*_L), ('bias', ctypes.c_void_p*_L),
        ('mean', ctypes.c_void_p), ('std', ctypes.c_void_p), ('mel_fwd', ctypes.c_void_p),
        ('mel_inv', ctypes.c_void_p)]


def _header_signatures():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f'{HEADER_PATH} is missing: the binding is derived from the C header')
    with open(HEADER_PATH) as f:
        return hip.parse_header(f.read())


# name -> (restype, argtypes) of every brv_ffs_* entry point, read from include/brever_ffnn_stream.h
SIGNATURES = _header_signatures()
_lib = None


def lib():
    """Load ``libbrever_ffnn_stream.so`` once; fail loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; '
                               'g.build()"` or `make -C brever_amd/csrc` (needs hipcc, targets gfx950). '
                               'FFNN streaming has no CPU fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


def last_error():
    msg = lib().brv_ffs_last_error()
    return msg.decode() if msg else ''


def call(name, *args):
    """Call the ``brv_ffs_*`` entry point ``name``; a non-zero status raises with the library's message."""
    status = getattr(_lib or lib(), name)(*args)
    if status:
        raise RuntimeError(f'{name} failed with status {status}: {last_error()}')


def query(name, *args):
    """Value of the int64_t size query ``name``; a negative one raises like ``call``."""
    n = getattr(_lib or lib(), name)(*args)
    if n < 0:
        raise RuntimeError(f'{name} failed with status {n}: {last_error()}')
    return int(n)
