"""ctypes binding of include/lidar4d_prep.h (liblidar4d_prep.so, gfx950): the point-cloud preparation kernels.

Same conventions as ``_lib`` (status -> HipExtensionError, ``*_workspace`` return int64, no CPU fallback), but a library of its
own that is loaded on FIRST USE, not at ``import lidar4d_amd``: a process that never prepares a point cloud maps
liblidar4d_hip.so only, and a missing liblidar4d_prep.so breaks nothing else.
"""
import ctypes as C
import os

from ._lib import HipExtensionError, P, I32, I64, F32, F64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_prep.so")
ABI_VERSION = 1
MAX_NEIGHBORS = 64

# name -> argtypes (all return int status, *_workspace int64); mirrors include/lidar4d_prep.h
SIGNATURES = {
    "l4dp_compact_workspace": [I64],
    "l4dp_range_filter": [P, I64, F32, F32, F32, F32, P, P, P, P, P],
    "l4dp_knn_workspace": [I64],
    "l4dp_knn_mean_dist": [P, I64, I32, P, P, P, P],
    "l4dp_outlier_filter": [P, P, I64, F64, P, P, P, P, P, P],
    "l4dp_plane_score": [P, I64, P, I32, F32, F32, P, P, P, P],
    "l4dp_plane_mask": [P, I64, P, I32, F32, P, P],
}

_lib = None


def lib():
    """Load liblidar4d_prep.so (once).  Raises HipExtensionError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C lidar4d_amd/csrc).  lidar4d_amd.pointprep has no CPU fallback.")
    l = C.CDLL(LIB_PATH)
    l.l4dp_version.restype = C.c_int
    l.l4dp_last_error.restype = C.c_char_p
    if l.l4dp_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI mismatch: library {l.l4dp_version()} != binding {ABI_VERSION}; rebuild")
    for name, args in SIGNATURES.items():
        fn = getattr(l, name)
        fn.argtypes = args
        fn.restype = C.c_int64 if name.endswith("_workspace") else C.c_int
    _lib = l
    return l


def call(name, *args):
    status = getattr(lib(), name)(*args)
    if status != 0:
        raise HipExtensionError(f"{name} failed: {lib().l4dp_last_error().decode()}")
