"""ctypes binding of include/lidar4d_planes.h (liblidar4d_planes.so, gfx950): the hex-plane sampler and the plane half of
``LiDAR4D.density`` for 4, 8 and 16 channels per plane (forward, and backward towards the planes, the flow and the coordinates).

Same conventions as ``_lib`` (status -> HipExtensionError, no CPU fallback), but a library of its own that is loaded on FIRST
USE, not at ``import lidar4d_amd``: a model of 8 channels per plane never maps it, and a missing liblidar4d_planes.so breaks
nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32, I64, PI32, PI64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_planes.so")
ABI_VERSION = 1

WIDTHS = (4, 8, 16)  # channels per plane of this library; the product path of 8 is liblidar4d_hip.so's (l4d_planes_*, the fused encode)

# name -> argtypes (all return int status); mirrors include/lidar4d_planes.h
_ARENA = [P, PI64, PI32, I32, I32]  # planes_cl, plane_off, res, n_scales, C
_FLOW = [P, I32, I32, P]            # flow, flow_stride, flow_half, tinfo
SIGNATURES = {
    "l4dh_planes_fwd": _ARENA + [P, I64, I32, P, P, P],
    "l4dh_planes_bwd": _ARENA + [P, I64, I32, P, P, P, P, P],
    "l4dh_density_planes_fwd": _ARENA + [P] + _FLOW + [I64, P, P, P],
    "l4dh_density_planes_bwd": _ARENA + [P] + _FLOW + [I64, P, P, P, P, P, P],
}

_binding = Binding(LIB_PATH, "l4dh_", ABI_VERSION, SIGNATURES,
                   "Planes4D with 4 or 16 channels per plane and Planes4D.density_features have no CPU fallback "
                   "(oracle/fields_ref.py is the torch restatement).")
lib, version, call = _binding.lib, _binding.version, _binding.call
