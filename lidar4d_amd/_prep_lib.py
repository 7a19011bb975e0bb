"""ctypes binding of include/lidar4d_prep.h (liblidar4d_prep.so, gfx950): the point-cloud preparation kernels.

Same conventions as ``_lib`` (status -> HipExtensionError, ``*_workspace`` return int64, no CPU fallback), but a library of its
own that is loaded on FIRST USE, not at ``import lidar4d_amd``: a process that never prepares a point cloud maps
liblidar4d_hip.so only, and a missing liblidar4d_prep.so breaks nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32, I64, F32, F64

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

_binding = Binding(LIB_PATH, "l4dp_", ABI_VERSION, SIGNATURES, "lidar4d_amd.pointprep has no CPU fallback.")
lib, version, call = _binding.lib, _binding.version, _binding.call
