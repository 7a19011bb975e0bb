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

// depth of sample ti of T along a ray (renderer.py:77-86); noise: null, or the ray's jitter value in [0, 1) for this sample
__device__ __forceinline__ float sample_depth(const float* __restrict__ lin, const float* __restrict__ noise, int ti, int T, float near,
                                              float far) {
  float z = near + (far - near) * lin[ti];
  if (noise) {
    const float sample_dist = (far - near) / (float)T;
    z = z + (*noise - 0.5f) * sample_dist;
  }
  return z;
}

// the (x, y, z, t) row the field kernels read for depth z on a ray (lidar4d.py:141,148-149)
__device__ __forceinline__ float4_t xt_row(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t ray, float z,
                                           float t, float bound) {
  float4_t o;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = unit_coord(ray_point(rays_o[ray * 3 + k], rays_d[ray * 3 + k], z, bound), bound);
  }
  o[3] = t;
  return o;
}

// renderer.py:98-110
__device__ __forceinline__ float alpha_of(float delta, float sigma, float density_scale, int active) {
  // 1 - exp(-deltas * density_scale * sigma)  /  1 - exp(-2 * deltas * density_scale * sigma)
  float e = active ? ((-2.0f * delta) * density_scale) * sigma : ((-delta) * density_scale) * sigma;
  return 1.0f - expf(e);
}
