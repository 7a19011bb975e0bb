"""ctypes binding of include/lidar4d_eval.h (liblidar4d_eval.so, gfx950): the evaluation meters' kernels.

Same conventions as ``_lib`` (status -> HipExtensionError, ``*_workspace`` return int64, no CPU fallback), but a library of its
own that is loaded on FIRST USE, not at ``import lidar4d_amd``: a process that never evaluates a frame does not map it,
and a missing liblidar4d_eval.so breaks nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32, F32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_eval.so")
ABI_VERSION = 1
SSIM_WINDOW = 7

# name -> argtypes (all return int status, *_workspace int64); mirrors include/lidar4d_eval.h
SIGNATURES = {
    "l4de_image_errors_workspace": [I32, I32],
    "l4de_image_errors": [P, P, I32, I32, F32, F32, P, P, P],
}

_binding = Binding(LIB_PATH, "l4de_", ABI_VERSION, SIGNATURES, "DepthMeter / IntensityMeter have no CPU fallback.")
lib, version, call = _binding.lib, _binding.version, _binding.call
