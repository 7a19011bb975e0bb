// Device functions of a ray's sample point and its alpha, shared by render.hip, fused.hip and raymarch.hip: one definition, so the
// rows of slab_rows_kernel are sample_rays_xt_kernel's bits and the march's transmittance is composite_fwd_kernel's.  Every
// translation unit is compiled with -ffp-contract=off.
#pragma once
#include "common.h"

// component k of o + d * z, clamped to the scene box (renderer.py:89)
__device__ __forceinline__ float ray_point(float o, float d, float z, float bound) {
  float v = o + d * z;
  v = fminf(fmaxf(v, -bound), bound);
  return v;
}

// box coordinate -> [0, 1] (lidar4d.py:141)
__device__ __forceinline__ float unit_coord(float v, float bound) { return (v + bound) / (2.0f * bound); }

// renderer.py:98-110
__device__ __forceinline__ float alpha_of(float delta, float sigma, float density_scale, int active) {
  // 1 - exp(-deltas * density_scale * sigma)  /  1 - exp(-2 * deltas * density_scale * sigma)
  float e = active ? ((-2.0f * delta) * density_scale) * sigma : ((-delta) * density_scale) * sigma;
  return 1.0f - expf(e);
}
