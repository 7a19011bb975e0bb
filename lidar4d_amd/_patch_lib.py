"""ctypes binding of include/lidar4d_patch.h (liblidar4d_patch.so, gfx950): the patch depth-gradient loss and its gradient.

Same conventions as ``_lib`` (status -> HipExtensionError, ``*_workspace`` return int64, no CPU fallback), but a library of its
own that is loaded on FIRST USE, not at ``import lidar4d_amd``: a run without patch epochs never maps it, and a missing
liblidar4d_patch.so breaks nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32, I64, F32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_patch.so")
ABI_VERSION = 1
MAX_PATCH_PIXELS = 1024  # L4DG_MAX_PATCH_PIXELS

KINDS = {"l1": 0, "mse": 1, "huber": 2, "cos": 3}                    # L4DG_L1 ... L4DG_COS
SOBEL, GRAD_LOSS, GRAD_NORM_SMOOTH, SPATIAL_SMOOTH, TV_LOSS = 1, 2, 4, 8, 16  # L4DG_* flag bits

# name -> argtypes (all return int status, *_workspace int64); mirrors include/lidar4d_patch.h
SIGNATURES = {
    "l4dg_patch_workspace": [I32, I32, I32],
    "l4dg_patch_fwd": [P, P, P, I32, I32, I32, I32, F32, I32, I32, F32, F32, F32, F32, P, P, P, P],
    "l4dg_patch_bwd": [P, P, I64, P, P],
}

_binding = Binding(LIB_PATH, "l4dg_", ABI_VERSION, SIGNATURES,
                   "patch_depth_grad_loss has no CPU fallback (trainer.depth_grad_loss is the torch restatement).")
lib, version, call = _binding.lib, _binding.version, _binding.call
