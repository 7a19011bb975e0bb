"""ctypes binding of include/lidar4d_march.h (liblidar4d_march.so, gfx950): the two kernels around a slab of the early-terminating
ray march (``render(..., early_stop=eps)``, lidar4d_amd/early_stop.py).

Same conventions as ``_lib`` (status -> HipExtensionError, no CPU fallback), but a library of its own that is loaded on FIRST USE,
not at ``import lidar4d_amd``: a render without ``early_stop`` never maps it, and a missing liblidar4d_march.so breaks nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32, I64, F32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_march.so")
ABI_VERSION = 1

# name -> argtypes (all return int status, *_workspace int64); mirrors include/lidar4d_march.h
SIGNATURES = {
    "l4dr_march_init": [I64, P, P, P, P],
    "l4dr_slab_rows": [P, P, P, P, P, I64, I64, I32, I32, I32, F32, F32, F32, P, P],
    "l4dr_slab_update_workspace": [I64],
    "l4dr_slab_update": [P, P, P, P, I64, I64, I32, I32, I32, F32, F32, I32, F32, P, P, P, P, P, P, P, P],
}

_binding = Binding(LIB_PATH, "l4dr_", ABI_VERSION, SIGNATURES,
                   "render(early_stop=...) has no CPU fallback (tests/early_stop_ref.py is the numpy restatement of its retirement rule).")
lib, version, call = _binding.lib, _binding.version, _binding.call
