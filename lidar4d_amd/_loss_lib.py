"""ctypes binding of include/lidar4d_loss.h (liblidar4d_loss.so, gfx950): the line-of-sight loss term and its gradient.

Same conventions as ``_lib`` (status -> HipExtensionError, ``*_workspace`` return int64, no CPU fallback), but a library of its
own that is loaded on FIRST USE, not at ``import lidar4d_amd``: a run without ``urf=True`` never maps it, and a missing
liblidar4d_loss.so breaks nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_loss.so")
ABI_VERSION = 1

# name -> argtypes (all return int status, *_workspace int64); mirrors include/lidar4d_loss.h
SIGNATURES = {
    "l4dl_los_workspace": [I32, I32],
    "l4dl_los_fwd": [P, P, P, I32, I32, I32, P, I32, I32, P, P, P],
    "l4dl_los_bwd": [P, P, P, I32, I32, I32, P, I32, I32, P, P, P, P],
}

_binding = Binding(LIB_PATH, "l4dl_", ABI_VERSION, SIGNATURES,
                   "line_of_sight_loss has no CPU fallback (trainer.urf_loss is the torch restatement).")
lib, version, call = _binding.lib, _binding.version, _binding.call
