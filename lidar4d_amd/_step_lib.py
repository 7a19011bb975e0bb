"""ctypes binding of include/lidar4d_step.h (liblidar4d_step.so, gfx950): the ray batch of a real sequence (patches expanded on the
device, ground truth in the frame's own dtype) and the primary losses for any criterion and fp32 or fp16 ground truth.

Same conventions as ``_lib`` (status -> HipExtensionError, ``*_workspace`` return int64, no CPU fallback), but a library of its
own that is loaded on FIRST USE, not at ``import lidar4d_amd``: the default fp32 step never maps it, and a missing
liblidar4d_step.so breaks nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32, F32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_step.so")
ABI_VERSION = 1

KINDS = {"l1": 0, "mse": 1, "bce": 2, "huber": 3}  # L4DS_L1 ... L4DS_HUBER

# name -> argtypes (all return int status, *_workspace int64); mirrors include/lidar4d_step.h
SIGNATURES = {
    "l4ds_ray_batch": [P, P, I32, I32, I32, P, F32, F32, I32, I32, P, I32, P, P, P, P, P],
    "l4ds_primary_losses_workspace": [I32],
    "l4ds_primary_losses": [P, P, P, I32, P, I32, I32, I32, I32, F32, F32, F32, F32, F32, F32, P, P, P, P, P, P, P],
}

_binding = Binding(LIB_PATH, "l4ds_", ABI_VERSION, SIGNATURES,
                   "ray_batch_patches / primary_losses_any have no CPU fallback (data.get_lidar_rays and trainer.lidar_loss are "
                   "the torch restatements).")
lib, version, call = _binding.lib, _binding.version, _binding.call
