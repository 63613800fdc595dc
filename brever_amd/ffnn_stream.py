"""ctypes binding of ``libbrever_ffnn_stream.so`` (C ABI ``brv_ffs_*``, ``include/brever_ffnn_stream.h``,
kernels under ``csrc/ffnn_stream/``): the streaming kernels of the FFNN mask estimator. A library of its own next
to ``libbrever_hip.so``, bound through ``hip.Library``: the table, the config struct and the limits are read from
the header, ``call`` / ``query`` raise with the library's own message. The streamer built on it is
``brever_amd.streaming.FFNNStreamer``. There is no CPU fallback.
"""
from . import hip

# the brv_ffs_* entry points of include/brever_ffnn_stream.h (a size query answers a Python int)
_LIB = hip.Library('brever_ffnn_stream.h', 'libbrever_ffnn_stream.so', 'BRV_FFS_LIB_PATH',
                   'FFNN streaming has no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, query, last_error = _LIB.lib, _LIB.call, _LIB.query, _LIB.last_error
# ``brv_ffs_config`` -- geometry of an FFNN and the addresses its values live at -- and the limits of its arrays
FfsConfig = _LIB.structs['brv_ffs_config']
MAX_HIDDEN, MAX_FEATURES = _LIB.constants['BRV_FFS_MAX_HIDDEN'], _LIB.constants['BRV_FFS_MAX_FEATURES']
