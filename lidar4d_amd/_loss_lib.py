"""ctypes binding of include/lidar4d_loss.h (liblidar4d_loss.so, gfx950): the line-of-sight loss term and its gradient.

Same conventions as ``_lib`` (status -> HipExtensionError, ``*_workspace`` return int64, no CPU fallback), but a library of its
own that is loaded on FIRST USE, not at ``import lidar4d_amd``: a run without ``urf=True`` never maps it, and a missing
liblidar4d_loss.so breaks nothing else.
"""
import ctypes as C
import os

from ._lib import HipExtensionError, P, I32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_loss.so")
ABI_VERSION = 1

# name -> argtypes (all return int status, *_workspace int64); mirrors include/lidar4d_loss.h
SIGNATURES = {
    "l4dl_los_workspace": [I32, I32],
    "l4dl_los_fwd": [P, P, P, I32, I32, I32, P, I32, I32, P, P, P],
    "l4dl_los_bwd": [P, P, P, I32, I32, I32, P, I32, I32, P, P, P, P],
}

_lib = None


def lib():
    """Load liblidar4d_loss.so (once).  Raises HipExtensionError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C lidar4d_amd/csrc).  line_of_sight_loss has no CPU fallback (trainer.urf_loss is the torch restatement).")
    l = C.CDLL(LIB_PATH)
    l.l4dl_version.restype = C.c_int
    l.l4dl_last_error.restype = C.c_char_p
    if l.l4dl_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI mismatch: library {l.l4dl_version()} != binding {ABI_VERSION}; rebuild")
    for name, args in SIGNATURES.items():
        fn = getattr(l, name)
        fn.argtypes = args
        fn.restype = C.c_int64 if name.endswith("_workspace") else C.c_int
    _lib = l
    return l


def call(name, *args):
    status = getattr(lib(), name)(*args)
    if status != 0:
        raise HipExtensionError(f"{name} failed: {lib().l4dl_last_error().decode()}")
