"""ctypes binding of ``libbrever_ffnn_stream.so`` (C ABI ``brv_ffs_*``, ``include/brever_ffnn_stream.h``,
kernels under ``csrc/ffnn_stream/``): the streaming kernels of the FFNN mask estimator. A library of its own next
to ``libbrever_hip.so``, bound through ``hip.Library``: the table is read from the header, ``call`` / ``query``
raise with the library's own message. The streamer built on it is
``brever_amd.streaming.FFNNStreamer``. There is no CPU fallback.
"""
import ctypes

from . import hip

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


# the brv_ffs_* entry points of include/brever_ffnn_stream.h (a size query answers a Python int)
_LIB = hip.Library('brever_ffnn_stream.h', 'libbrever_ffnn_stream.so', 'BRV_FFS_LIB_PATH',
                   'FFNN streaming has no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, query, last_error = _LIB.lib, _LIB.call, _LIB.query, _LIB.last_error
