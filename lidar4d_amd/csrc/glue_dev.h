// What csrc/glue.hip (liblidar4d_hip.so) and csrc/stepglue.hip (liblidar4d_step.so) share: the fixed-order sum of a 256-thread
// workgroup and the one-workgroup sum of the per-workgroup partials.  One definition, so that the primary losses
// (l4ds_primary_losses) and the ray-chamfer term added to them (l4d_ray_chamfer_grad) reduce in one fixed order, the one
// tests/realdata_cases.py fixed_order_sum restates.
#pragma once
#include "common.h"

// fixed-order sum of one value per thread over a 256-thread workgroup
__device__ __forceinline__ float block_sum_256(float v, float* red /* [256] */) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// loss[0] = (accumulate ? loss[0] : 0) + coef * (partial[0] + partial[1] + ...), summed in index order by one workgroup: the
// per-block partial sums of the loss kernels become ONE number that is the same every run (no floating-point atomics)
__global__ void __launch_bounds__(256) sum_partials_kernel(const float* __restrict__ partial, int n, float coef, int accumulate,
                                                           float* __restrict__ loss) {
  __shared__ float red[256];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  const float total = block_sum_256(acc, red);
  if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.0f) + coef * total;
}
