"""ctypes binding of include/lidar4d_mlp.h (liblidar4d_mlp.so, gfx950): the fused bias-free ReLU MLP for the hidden widths 16, 32
and 128 (forward with the optional density activation epilogue, backward with accumulated weight gradients).

Same conventions as ``_lib`` (status -> HipExtensionError, no CPU fallback), but a library of its own that is loaded on FIRST
USE, not at ``import lidar4d_amd``: a model whose networks are all 64 wide never maps it, and a missing liblidar4d_mlp.so breaks
nothing else.
"""
import os

from ._lib import Binding, HipExtensionError, P, I32, I64, F32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblidar4d_mlp.so")
ABI_VERSION = 1

WIDTHS = (16, 32, 128)  # hidden widths of this library; 64 is liblidar4d_hip.so's (l4d_mlp_*)

# name -> argtypes (all return int status); mirrors include/lidar4d_mlp.h
SIGNATURES = {
    "l4dm_mlp_fwd": [P, I64, P, I32, I32, I32, P, P, P, P, P],
    "l4dm_mlp_bwd": [P, P, P, I64, P, I32, I32, I32, P, P, P, F32, P, I32, I32, P],
}

_binding = Binding(LIB_PATH, "l4dm_", ABI_VERSION, SIGNATURES,
                   "mlp_fwd / mlp_bwd / mlp_fwd_sigma with hidden in (16, 32, 128) have no CPU fallback (oracle/tcnn_ref.py is "
                   "the torch restatement).")
lib, version, call = _binding.lib, _binding.version, _binding.call
