// The two ends of a training step (include/lidar4d_step.h, liblidar4d_step.so): the ray batch and the primary losses of every
// dataset and criterion set, ONE sweep over the rays each.
//
//   l4ds_ray_batch        drawn patch corners -> pixel indices, rays_o / rays_d, and the drawn pixels' ground truth in the frame's own
//                         type (the reference preloads fp16: data/kitti360_dataset.py:141-147); the px x py patch is expanded
//                         in the kernel (data/base_dataset.py:36-70)
//   l4ds_primary_losses   runner.py:179-213 for any of the four criteria per term and fp32 or fp16 ground truth: value,
//                         gradients, optionally the ray-chamfer term's point sets and an fp32 copy of the ground truth
//
// Both stream over n rays, a thread per ray, 12 to 60 bytes each way: nothing to stage, the only LDS is the workgroup sum.  All
// arithmetic is written in the reference's operation order (this file is compiled without fma contraction) and the loss is summed
// in two fixed-order stages (glue_dev.h): the same input gives the same bits, and the L1 / MSE / MSE case on fp32 ground truth
// those of a numpy float32 evaluation in the same order (tests/realdata_cases.py primary_losses_ref).
#include <stdio.h>

#include "common.h"
#include "glue_dev.h"
#include "../../include/lidar4d_step.h"

extern "C" int l4ds_version(void) { return L4DS_ABI_VERSION; }
extern "C" const char* l4ds_last_error(void) { return l4d_last_error(); }

static int step_fail(const char* who, const char* what) {
  static thread_local char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  l4d_set_error(1, msg);
  return 1;
}

// ---- ray batch -------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) step_ray_batch_kernel(const int64_t* __restrict__ top, const int64_t* __restrict__ left, int n,
                                                             int px, int py, const float* __restrict__ pose, float fov_up, float fov,
                                                             int H, int W, const T* __restrict__ image, float* __restrict__ rays_o,
                                                             float* __restrict__ rays_d, T* __restrict__ gt,
                                                             int64_t* __restrict__ inds) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int patch = k / (px * py), rem = k - patch * (px * py);
  const int pr = rem / py, pc = rem - pr * py;
  const int64_t r = top[patch] + pr;
  int64_t c = (left[patch] + pc) % W;  // (the panorama wraps around)
  if (c < 0) c += W;
  const int64_t ind = r * W + c;
  inds[k] = ind;
  // base_dataset.py:82-93: i = column, j = row (floats); beta = -(i - W/2) / W * 2 * pi; alpha = (fov_up - j / H * fov) / 180 * pi
  const float i = (float)c, j = (float)r;
  const float pi = 3.14159265358979323846f;
  const float beta = -(i - (float)((double)W / 2.0)) / (float)W * 2.0f * pi;
  const float alpha = (fov_up - j / (float)H * fov) / 180.0f * pi;
  const float ca = cosf(alpha), sa = sinf(alpha), cb = cosf(beta), sb = sinf(beta);
  const float d[3] = {ca * cb, ca * sb, sa};
#pragma unroll
  for (int a = 0; a < 3; ++a) {  // rays_d = directions @ R^T, rays_o = translation
    rays_d[k * 3 + a] = d[0] * pose[a * 4 + 0] + d[1] * pose[a * 4 + 1] + d[2] * pose[a * 4 + 2];
    rays_o[k * 3 + a] = pose[a * 4 + 3];
  }
  if (image) {
    const bool inside = r >= 0 && r < H;
#pragma unroll
    for (int a = 0; a < 3; ++a) gt[k * 3 + a] = inside ? image[ind * 3 + a] : (T)0.0f;
  }
}

extern "C" int l4ds_ray_batch(const int64_t* top, const int64_t* left, int32_t n_patch, int32_t px, int32_t py, const float* pose,
                              float fov_up, float fov, int32_t H, int32_t W, const void* image, int32_t image_half, float* rays_o,
                              float* rays_d, void* gt, int64_t* inds, void* stream_) {
  const char* who = "l4ds_ray_batch";
  hipStream_t stream = (hipStream_t)stream_;
  if (n_patch < 0) return step_fail(who, "negative patch count");
  if (px < 1 || py < 1) return step_fail(who, "a patch side must be at least 1");
  if (H <= 0 || W <= 0) return step_fail(who, "empty image (H and W must be at least 1)");
  const int64_t n = (int64_t)n_patch * px * py;
  if (n >= ((int64_t)1 << 31) / 3) return step_fail(who, "too many rays (3 n must stay below 2^31)");
  if ((int64_t)H * W >= ((int64_t)1 << 31) / 3) return step_fail(who, "image too large (3 H W must stay below 2^31)");
  if (n == 0) return 0;
  if (!top || !left || !pose || !rays_o || !rays_d || !inds || (image && !gt)) return step_fail(who, "null pointer");
  const dim3 grid((unsigned)ceil_div64(n, 256)), block(256);
  if (image_half)
    L4D_LAUNCH(step_ray_batch_kernel<half_t>, grid, block, 0, stream, top, left, (int)n, (int)px, (int)py, pose, fov_up, fov, (int)H,
               (int)W, (const half_t*)image, rays_o, rays_d, (half_t*)gt, inds);
  else
    L4D_LAUNCH(step_ray_batch_kernel<float>, grid, block, 0, stream, top, left, (int)n, (int)px, (int)py, pose, fov_up, fov, (int)H,
               (int)W, (const float*)image, rays_o, rays_d, (float*)gt, inds);
  L4D_LAUNCH_CHECK(who);
  return 0;
}

// ---- primary losses --------------------------------------------------------------------------------------------------------
// One criterion at prediction a and target b: the value, and dv = d value / d a as autograd gives it.
__device__ __forceinline__ float step_criterion(int kind, float a, float b, float delta, float& dv) {
  const float e = a - b;
  switch (kind) {
    case L4DS_L1:
      dv = e > 0.0f ? 1.0f : e < 0.0f ? -1.0f : 0.0f;
      return fabsf(e);
    case L4DS_MSE:
      dv = 2.0f * e;
      return e * e;
    case L4DS_HUBER: {
      const float z = fabsf(e);
      dv = e < -delta ? -delta : e > delta ? delta : e;
      return z < delta ? 0.5f * z * z : delta * (z - 0.5f * delta);
    }
    default: {  // L4DS_BCE with logits: (1 - b) * a - log_sigmoid(a), log_sigmoid(a) = min(a, 0) - log1p(exp(-|a|))
      dv = 1.0f / (1.0f + expf(-a)) - b;
      return (1.0f - b) * a - (fminf(a, 0.0f) - log1pf(expf(-fabsf(a))));
    }
  }
}

struct StepKinds {
  int depth, raydrop, intensity;
};

// a ray's ground truth as the loss sees it: mask, masked intensity and depth, smoothed mask, and the three raw channels
struct StepGt {
  float m, gt_i, gt_d, gs, raw[3];
};
template <bool HALF>
__device__ __forceinline__ StepGt step_gt(const void* __restrict__ gt, int k, float smooth) {
  StepGt g;
  if constexpr (HALF) {  // torch's half arithmetic: each product and the clamp in fp32, rounded to half; then widened exactly
    const half_t* h = (const half_t*)gt + (size_t)k * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) g.raw[a] = h2f(h[a]);
    g.m = g.raw[0];
    g.gt_i = h2f(f2h(g.raw[1] * g.m));
    g.gt_d = h2f(f2h(g.raw[2] * g.m));
    const float lo = h2f(f2h(smooth)), hi = h2f(f2h(1.0f - smooth));
    g.gs = fminf(fmaxf(g.m, lo), hi);
  } else {
    const float* f = (const float*)gt + (size_t)k * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) g.raw[a] = f[a];
    g.m = g.raw[0];
    g.gt_i = g.raw[1] * g.m;
    g.gt_d = g.raw[2] * g.m;
    g.gs = fminf(fmaxf(g.m, smooth), 1.0f - smooth);
  }
  return g;
}

template <bool HALF>
__global__ void __launch_bounds__(256) step_primary_losses_kernel(const float* __restrict__ depth, const float* __restrict__ image,
                                                                  const void* __restrict__ gt, const float* __restrict__ rays_d, int n,
                                                                  StepKinds kinds, float alpha_d, float alpha_r, float alpha_i,
                                                                  float smooth, float delta, float scale, float* __restrict__ partial,
                                                                  float* __restrict__ g_depth, float* __restrict__ g_image,
                                                                  float* __restrict__ pts, float* __restrict__ gt32) {
  __shared__ float red[256];
  float acc = 0.0f;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    const StepGt g = step_gt<HALF>(gt, k, smooth);
    const float m = g.m;
    float p_r = image[k * 2 + 0];
    const float p_i = image[k * 2 + 1] * m, p_d = depth[k] * m;
    float chain_r = 1.0f;  // d p_r / d image[0]
    if (kinds.raydrop == L4DS_BCE) {  // runner.py:197-198: the sigmoid in front of BCE-with-logits
      p_r = 1.0f / (1.0f + expf(-p_r));
      chain_r = (1.0f - p_r) * p_r;
    }
    float dv_d, dv_r, dv_i;
    const float v_d = step_criterion(kinds.depth, p_d, g.gt_d, delta, dv_d);
    const float v_r = step_criterion(kinds.raydrop, p_r, g.gs, delta, dv_r);
    const float v_i = step_criterion(kinds.intensity, p_i, g.gt_i, delta, dv_i);
    acc = alpha_d * v_d + alpha_r * v_r + alpha_i * v_i;
    g_depth[k] = alpha_d * dv_d * m;
    g_image[k * 2 + 0] = kinds.raydrop == L4DS_BCE ? alpha_r * dv_r * chain_r : alpha_r * dv_r;
    g_image[k * 2 + 1] = alpha_i * dv_i * m;
    if (pts) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float rd = rays_d[k * 3 + a];
        pts[k * 3 + a] = rd * p_d / scale;
        pts[(n + k) * 3 + a] = rd * g.gt_d / scale;
      }
    }
    if (gt32) {
#pragma unroll
      for (int a = 0; a < 3; ++a) gt32[k * 3 + a] = g.raw[a];
    }
  }
  const float total = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

extern "C" int64_t l4ds_primary_losses_workspace(int32_t n) { return n < 0 ? 0 : 4 * (int64_t)(n > 0 ? (n + 255) / 256 : 1); }

extern "C" int l4ds_primary_losses(const float* depth, const float* image, const void* gt, int32_t gt_half, const float* rays_d, int32_t n,
                                   int32_t kind_depth, int32_t kind_raydrop, int32_t kind_intensity, float alpha_d, float alpha_r,
                                   float alpha_i, float smooth, float delta, float scale, float* loss_out, float* g_depth_out,
                                   float* g_image_out, float* pts_out, float* gt32_out, void* workspace, void* stream_) {
  const char* who = "l4ds_primary_losses";
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0) return step_fail(who, "negative ray count");
  if (n >= (1 << 30) / 3) return step_fail(who, "too many rays (6 n must stay below 2^31)");
  for (int32_t kind : {kind_depth, kind_raydrop, kind_intensity})
    if (kind < L4DS_L1 || kind > L4DS_HUBER) return step_fail(who, "unknown criterion (L4DS_L1, L4DS_MSE, L4DS_BCE, L4DS_HUBER)");
  if (!loss_out || !workspace) return step_fail(who, "null pointer");
  if (n > 0 && (!depth || !image || !gt || !g_depth_out || !g_image_out || (pts_out && !rays_d))) return step_fail(who, "null pointer");
  if (((uintptr_t)workspace & 3) != 0) return step_fail(who, "workspace must be 4-byte aligned");
  const int blocks = (n + 255) / 256;
  float* partial = (float*)workspace;
  const StepKinds kinds = {(int)kind_depth, (int)kind_raydrop, (int)kind_intensity};
  if (blocks > 0) {
    if (gt_half)
      L4D_LAUNCH(step_primary_losses_kernel<true>, dim3(blocks), dim3(256), 0, stream, depth, image, gt, rays_d, (int)n, kinds, alpha_d,
                 alpha_r, alpha_i, smooth, delta, scale, partial, g_depth_out, g_image_out, pts_out, gt32_out);
    else
      L4D_LAUNCH(step_primary_losses_kernel<false>, dim3(blocks), dim3(256), 0, stream, depth, image, gt, rays_d, (int)n, kinds, alpha_d,
                 alpha_r, alpha_i, smooth, delta, scale, partial, g_depth_out, g_image_out, pts_out, gt32_out);
  }
  L4D_LAUNCH(sum_partials_kernel, dim3(1), dim3(256), 0, stream, (const float*)partial, blocks, 1.0f, 0, loss_out);
  L4D_LAUNCH_CHECK(who);
  return 0;
}
