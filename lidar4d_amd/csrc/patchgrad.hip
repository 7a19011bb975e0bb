// The patch depth-gradient loss (include/lidar4d_patch.h, liblidar4d_patch.so): what the reference's patch epochs add to the
// training loss (model/runner.py:277-369) and what torch evaluates with about forty element-wise launches forward and as many
// backward on a [1, n] vector, as one sweep that leaves the value's partials AND the gradient, one launch that adds the
// partials, and -- in the backward -- one launch that scales the gradient.
//
//   sweep   : a workgroup takes a GROUP of whole patches at a time and strides over the groups.  While px * py <= 64 a wavefront
//             holds 64 / (px * py) patches, one pixel per lane (a group = 4 wavefronts' patches); a larger patch is a group of its
//             own and the workgroup's threads stride over its pixels.  Per group, through LDS:
//               load      p = pred * (1 / scale), q = gt * (1 / scale), hit                       -> s_p, s_q, s_h
//               respond   every pixel: the x and y responses at its position (forward difference or Sobel), the value they
//                         contribute (fp64, per thread), and cx = d loss / d rx, cy = d loss / d ry        -> s_cx, s_cy
//               (cos)     the patch's three sums |a|^2, |b|^2, a.b -- a serial fp64 loop over the patch's LDS image inside the
//                         wavefront, or three workgroup reductions for a large patch -- and the criterion's share of cx
//               gather    every pixel collects the cx / cy of the differences or stencil taps it takes part in and writes its
//                         element of the gradient: no scatter, no atomics
//             then one fp64 partial per workgroup.
//   finish  : one workgroup adds the partials in a fixed order and writes the loss.
//   scale   : d_pred = g[0] * g_pred.
// Element-wise arithmetic is fp32 in torch's order (the library is compiled with -ffp-contract=off), so masks, signs and Huber
// branches are torch's; the divisors of the means are known from the shape, which is why the gradient needs no second sweep.
// `x / scale` with a python float is evaluated by torch ON THE DEVICE as x * (1.0f / scale) -- forward and in autograd's backward
// (measured on MI355X, torch 2.10: 65,536 of 65,536 elements equal the product, 35,948 the quotient) -- and so it is here: with
// the quotient, one unit in the last place of a 30 m depth (2e-6) is 1e-3 of a 2 mm difference, far beyond the 2e-5 bound against
// the restatement.  For fp16 ground truth both forms round to the same half.
#include <stdio.h>

#include "common.h"
#include "wave_dev.h"
#include "../../include/lidar4d_patch.h"

extern "C" int l4dg_version(void) { return L4DG_ABI_VERSION; }
extern "C" const char* l4dg_last_error(void) { return l4d_last_error(); }

#define PG_THREADS 256
#define PG_WAVES (PG_THREADS / L4D_WAVE)
#define PG_MAX_PIX L4DG_MAX_PATCH_PIXELS  // pixels of a group: one large patch, or at most 4 wavefronts x 64 lanes
#define PG_MAX_BLOCKS 1024                // the grid, and so the number of partials, is bounded; workgroups stride over the groups

struct PgArgs {
  const float* pred;
  const void* gt;
  const void* hit;
  int gt_half, n_patch, px, py, kind, flags;
  float inv_scale;  // 1.0f / scale
  float delta;      // (float)(0.2 * scale)
  float cn_x, cn_y, cs_x, cs_y, ct_x, ct_y;  // alpha / (number of elements of the x / y difference image), fp32 as autograd has it
  double wn_x, wn_y, ws_x, ws_y, wt_x, wt_y;  // the same weights for the value
  float alpha_grad;
};

__device__ __forceinline__ float pg_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ float pg_load(const void* __restrict__ p, int half, int64_t i) {
  return half ? h2f(((const half_t*)p)[i]) : ((const float*)p)[i];
}

// One item of a group: which patch slot of the group, which pixel of the patch, where in the group's LDS image.
struct PgItem {
  int slot, pix, li;
  bool valid;
};
template <bool BIG>
__device__ __forceinline__ PgItem pg_item(int e, int P, int per_wave, int64_t patch0, int n_patch) {
  PgItem it;
  if (BIG) {
    it.slot = 0, it.pix = e, it.li = e, it.valid = e < P;
  } else {
    const int wave = e >> 6, lane = e & 63;
    const int sub = lane / P;
    it.slot = wave * per_wave + sub;
    it.pix = lane - sub * P;
    it.li = it.slot * P + it.pix;
    it.valid = sub < per_wave && patch0 + it.slot < n_patch;
  }
  return it;
}

// What a pixel's position contributes: the signed x / y responses of the prediction, whether the position exists in the x / y
// difference image, and the main term's operands a, b with fa = d a / d rx.
struct PgResp {
  float rx, ry, a, b, fa;
  bool vx, vy;
};
__device__ __forceinline__ float pg_sobel(const float* __restrict__ img, int px, int py, int i, int j, bool along_x) {
  float r = 0.0f;
#pragma unroll
  for (int u = -1; u <= 1; ++u) {
#pragma unroll
    for (int v = -1; v <= 1; ++v) {
      const int k = along_x ? v * (u == 0 ? 2 : 1) : u * (v == 0 ? 2 : 1);
      const int ii = i + u, jj = j + v;
      if (k != 0 && ii >= 0 && ii < px && jj >= 0 && jj < py) r += (float)k * img[ii * py + jj];
    }
  }
  return r;
}
__device__ __forceinline__ PgResp pg_respond(const PgArgs& A, const float* __restrict__ sp, const float* __restrict__ sq,
                                             const float* __restrict__ sh, int pix) {
  const int px = A.px, py = A.py, i = pix / py, j = pix - i * py;
  const bool sobel = (A.flags & L4DG_SOBEL) != 0;
  PgResp r;
  float ggx = 0.0f;
  if (sobel) {
    r.vx = r.vy = true;
    r.rx = pg_sobel(sp, px, py, i, j, true);
    r.ry = pg_sobel(sp, px, py, i, j, false);
    if (A.flags & L4DG_GRAD_LOSS) ggx = pg_sobel(sq, px, py, i, j, true);
  } else {
    r.vx = j < py - 1, r.vy = i < px - 1;
    r.rx = r.vx ? sp[pix] - sp[pix + 1] : 0.0f;
    r.ry = r.vy ? sp[pix] - sp[pix + py] : 0.0f;
    if ((A.flags & L4DG_GRAD_LOSS) && r.vx) {
      ggx = sq[pix] - sq[pix + 1];
      if (A.gt_half) ggx = h2f(f2h(ggx));
    }
  }
  r.a = r.b = r.fa = 0.0f;
  if ((A.flags & L4DG_GRAD_LOSS) && r.vx) {
    const float mask = sh[pix] * (fabsf(ggx) < 0.01f ? 1.0f : 0.0f);
    r.a = (sobel ? r.rx : fabsf(r.rx)) * mask;
    r.b = ggx * mask;
    if (A.gt_half) r.b = h2f(f2h(r.b));
    r.fa = sobel ? mask : mask * pg_sign(r.rx);
  }
  return r;
}

template <bool BIG>
__global__ void __launch_bounds__(PG_THREADS) pg_sweep_kernel(PgArgs A, double* __restrict__ partial, float* __restrict__ g_pred) {
  __shared__ float s_p[PG_MAX_PIX], s_q[PG_MAX_PIX], s_h[PG_MAX_PIX], s_cx[PG_MAX_PIX], s_cy[PG_MAX_PIX], s_a[PG_MAX_PIX], s_b[PG_MAX_PIX];
  __shared__ double sh_sum[PG_WAVES];
  const int P = A.px * A.py, py = A.py, px = A.px;
  const int per_wave = BIG ? 0 : 64 / P;
  const int per_group = BIG ? 1 : per_wave * PG_WAVES;
  const int span = BIG ? P : PG_THREADS;  // items of a group (BIG: the patch's pixels; else one per thread)
  const int64_t n_groups = ((int64_t)A.n_patch + per_group - 1) / per_group;
  const bool main_term = (A.flags & L4DG_GRAD_LOSS) != 0, cosine = main_term && A.kind == L4DG_COS;
  const bool sobel = (A.flags & L4DG_SOBEL) != 0;
  double acc = 0.0;
  for (int64_t group = blockIdx.x; group < n_groups; group += gridDim.x) {  // (the same trips for every thread of the workgroup)
    const int64_t patch0 = group * per_group;
    // ---- load ----
    for (int e = threadIdx.x; e < span; e += PG_THREADS) {
      const PgItem it = pg_item<BIG>(e, P, per_wave, patch0, A.n_patch);
      if (!it.valid) continue;
      const int64_t gi = (patch0 + it.slot) * P + it.pix;
      s_p[it.li] = A.pred[gi] * A.inv_scale;
      if (main_term) {
        float q = pg_load(A.gt, A.gt_half, gi) * A.inv_scale;
        if (A.gt_half) q = h2f(f2h(q));
        s_q[it.li] = q;
        s_h[it.li] = pg_load(A.hit, A.gt_half, gi);
      }
    }
    __syncthreads();
    // ---- respond ----
    double ca = 0.0, cb = 0.0, cd = 0.0;  // (BIG, cos) this thread's share of the patch's three sums
    for (int e = threadIdx.x; e < span; e += PG_THREADS) {
      const PgItem it = pg_item<BIG>(e, P, per_wave, patch0, A.n_patch);
      if (!it.valid) continue;
      const int base = it.li - it.pix;
      const PgResp r = pg_respond(A, s_p + base, s_q + base, s_h + base, it.pix);
      float cx = 0.0f, cy = 0.0f;  // d loss / d |rx|, d loss / d |ry| of the smoothness terms
      if (r.vx) {
        const float dx = fabsf(r.rx);
        if (A.flags & L4DG_GRAD_NORM_SMOOTH) {
          const float ex = expf(-dx);
          acc += A.wn_x * (double)ex;
          cx += -(A.cn_x * ex);
        }
        if (A.flags & L4DG_SPATIAL_SMOOTH) {
          acc += A.ws_x * (double)(dx * dx);
          cx += A.cs_x * (2.0f * dx);
        }
        if (A.flags & L4DG_TV_LOSS) {
          acc += A.wt_x * (double)dx;
          cx += A.ct_x;
        }
        cx *= pg_sign(r.rx);
      }
      if (r.vy) {
        const float dy = fabsf(r.ry);
        if (A.flags & L4DG_GRAD_NORM_SMOOTH) {
          const float ey = expf(-dy);
          acc += A.wn_y * (double)ey;
          cy += -(A.cn_y * ey);
        }
        if (A.flags & L4DG_SPATIAL_SMOOTH) {
          acc += A.ws_y * (double)(dy * dy);
          cy += A.cs_y * (2.0f * dy);
        }
        if (A.flags & L4DG_TV_LOSS) {
          acc += A.wt_y * (double)dy;
          cy += A.ct_y;
        }
        cy *= pg_sign(r.ry);
      }
      if (main_term && !cosine && r.vx) {
        const float d = r.a - r.b;
        float t, dt;  // the criterion and its derivative wrt a
        if (A.kind == L4DG_L1) {
          t = fabsf(d), dt = pg_sign(d);
        } else if (A.kind == L4DG_MSE) {
          t = d * d, dt = 2.0f * d;
        } else {
          const float z = fabsf(d);
          t = z < A.delta ? 0.5f * z * z : A.delta * (z - 0.5f * A.delta);
          dt = z < A.delta ? d : A.delta * pg_sign(d);
        }
        acc += (double)A.alpha_grad * (double)t;
        cx += (A.alpha_grad * dt) * r.fa;
      }
      if (cosine) {
        s_a[it.li] = r.a, s_b[it.li] = r.b;
        if (BIG) ca += (double)r.a * (double)r.a, cb += (double)r.b * (double)r.b, cd += (double)r.a * (double)r.b;
      }
      s_cx[it.li] = cx, s_cy[it.li] = cy;
    }
    __syncthreads();
    // ---- the cosine criterion: per patch ----
    if (cosine) {
      if (BIG) {
        ca = block_reduce<PG_WAVES>(ca, sh_sum, RedSum());
        cb = block_reduce<PG_WAVES>(cb, sh_sum, RedSum());
        cd = block_reduce<PG_WAVES>(cd, sh_sum, RedSum());
      }
      for (int e = threadIdx.x; e < span; e += PG_THREADS) {
        const PgItem it = pg_item<BIG>(e, P, per_wave, patch0, A.n_patch);
        if (!it.valid) continue;
        const int base = it.li - it.pix;
        if (!BIG) {  // every lane of the patch walks the patch's image in the same order: the same sums in each of them
          ca = cb = cd = 0.0;
          for (int k = 0; k < P; ++k) {
            const double a = (double)s_a[base + k], b = (double)s_b[base + k];
            ca += a * a, cb += b * b, cd += a * b;
          }
        }
        const double ra = sqrt(ca), rb = sqrt(cb);
        const double na = ra > 1e-8 ? ra : 1e-8, nb = rb > 1e-8 ? rb : 1e-8;
        if (it.pix == 0) acc += (double)A.alpha_grad * (1.0 - cd / (na * nb));
        const double a = (double)s_a[it.li], b = (double)s_b[it.li];
        double dcos = b / (na * nb);                          // d cos / d a of this element ...
        if (ra > 1e-8) dcos -= cd * a / (nb * na * na * ra);  // ... and through the norm of a (none through the 1e-8 floor)
        const PgResp r = pg_respond(A, s_p + base, s_q + base, s_h + base, it.pix);
        s_cx[it.li] += (float)(-(double)A.alpha_grad * dcos) * r.fa;
      }
      __syncthreads();
    }
    // ---- gather ----
    for (int e = threadIdx.x; e < span; e += PG_THREADS) {
      const PgItem it = pg_item<BIG>(e, P, per_wave, patch0, A.n_patch);
      if (!it.valid) continue;
      const int base = it.li - it.pix, i = it.pix / py, j = it.pix - i * py;
      const float* __restrict__ cx = s_cx + base;
      const float* __restrict__ cy = s_cy + base;
      float g = 0.0f;
      if (sobel) {  // the response at (i - u, j - v) read this pixel with the weight k(u, v)
#pragma unroll
        for (int u = -1; u <= 1; ++u) {
#pragma unroll
          for (int v = -1; v <= 1; ++v) {
            const int ii = i - u, jj = j - v;
            if (ii < 0 || ii >= px || jj < 0 || jj >= py) continue;
            const int kx = v * (u == 0 ? 2 : 1), ky = u * (v == 0 ? 2 : 1);
            if (kx != 0) g += (float)kx * cx[ii * py + jj];
            if (ky != 0) g += (float)ky * cy[ii * py + jj];
          }
        }
      } else {  // rx(i,j) = p(i,j) - p(i,j+1): + at its own position, - at the position to the left; ry likewise
        if (j < py - 1) g += cx[it.pix];
        if (j > 0) g -= cx[it.pix - 1];
        if (i < px - 1) g += cy[it.pix];
        if (i > 0) g -= cy[it.pix - py];
      }
      g_pred[(patch0 + it.slot) * P + it.pix] = g * A.inv_scale;
    }
    __syncthreads();  // (the next group overwrites the images)
  }
  acc = block_reduce<PG_WAVES>(acc, sh_sum, RedSum());
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(PG_THREADS) pg_finish_kernel(const double* __restrict__ partial, int n_part, float* __restrict__ loss_out) {
  __shared__ double sh_sum[PG_WAVES];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += PG_THREADS) s += partial[i];
  s = block_reduce<PG_WAVES>(s, sh_sum, RedSum());
  if (threadIdx.x == 0) loss_out[0] = (float)s;
}

__global__ void __launch_bounds__(PG_THREADS) pg_scale_kernel(const float* __restrict__ g_pred, const float* __restrict__ g, int64_t n,
                                                             float* __restrict__ d_pred) {
  const float s = g[0];
  for (int64_t i = (int64_t)blockIdx.x * PG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PG_THREADS) d_pred[i] = s * g_pred[i];
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
static const char* pg_shape_error(int32_t n_patch, int32_t px, int32_t py) {
  if (n_patch < 1) return "n_patch must be at least 1";
  if (px < 2 || py < 2) return "px and py must be at least 2";
  if ((int64_t)px * py > L4DG_MAX_PATCH_PIXELS) return "px * py must be at most 1024";
  if ((int64_t)n_patch * px * py > 0x7fffffffLL) return "n_patch * px * py must be below 2^31";
  return nullptr;
}

extern "C" int64_t l4dg_patch_workspace(int32_t n_patch, int32_t px, int32_t py) {
  return pg_shape_error(n_patch, px, py) ? 0 : (int64_t)PG_MAX_BLOCKS * 8;
}

extern "C" int l4dg_patch_fwd(const float* pred, const void* gt, const void* hit, int32_t gt_half, int32_t n_patch, int32_t px,
                              int32_t py, float scale, int32_t kind, int32_t flags, float alpha_grad, float alpha_grad_norm,
                              float alpha_spatial, float alpha_tv, float* loss_out, float* g_pred_out, void* workspace, void* stream_) {
  static thread_local char msg[160];
  hipStream_t stream = (hipStream_t)stream_;
  const char* what = pg_shape_error(n_patch, px, py);
  const int all_flags = L4DG_SOBEL | L4DG_GRAD_LOSS | L4DG_GRAD_NORM_SMOOTH | L4DG_SPATIAL_SMOOTH | L4DG_TV_LOSS;
  if (!what && (kind < L4DG_L1 || kind > L4DG_COS)) what = "unknown kind (0 l1, 1 mse, 2 huber, 3 cos)";
  if (!what && (flags & ~all_flags)) what = "unknown flag bits";
  if (!what && gt_half != 0 && (flags & L4DG_SOBEL)) what = "fp16 ground truth only with forward differences";
  if (!what && !(scale > 0.0f)) what = "scale must be positive";
  if (!what && (!pred || !loss_out || !g_pred_out || !workspace || ((flags & L4DG_GRAD_LOSS) && (!gt || !hit)))) what = "null pointer";
  if (!what && ((uintptr_t)workspace & 7) != 0) what = "workspace must be 8-byte aligned";
  if (what) {
    snprintf(msg, sizeof msg, "l4dg_patch_fwd: %s", what);
    L4D_FAIL(msg);
  }
  const int P = px * py;
  const bool big = P > 64;
  const int per_group = big ? 1 : (64 / P) * PG_WAVES;
  const int64_t n_groups = ceil_div64(n_patch, per_group);
  const int blocks = (int)(n_groups < PG_MAX_BLOCKS ? n_groups : PG_MAX_BLOCKS);
  const double n_x = (double)n_patch * ((flags & L4DG_SOBEL) ? (double)P : (double)px * (py - 1));
  const double n_y = (double)n_patch * ((flags & L4DG_SOBEL) ? (double)P : (double)(px - 1) * py);
  PgArgs A;
  A.pred = pred, A.gt = gt, A.hit = hit;
  A.gt_half = gt_half != 0, A.n_patch = n_patch, A.px = px, A.py = py, A.kind = kind, A.flags = flags;
  A.inv_scale = 1.0f / scale;
  A.delta = (float)(0.2 * (double)scale);
  A.cn_x = alpha_grad_norm / (float)n_x, A.cn_y = alpha_grad_norm / (float)n_y;
  A.cs_x = alpha_spatial / (float)n_x, A.cs_y = alpha_spatial / (float)n_y;
  A.ct_x = alpha_tv / (float)n_x, A.ct_y = alpha_tv / (float)n_y;
  A.wn_x = (double)alpha_grad_norm / n_x, A.wn_y = (double)alpha_grad_norm / n_y;
  A.ws_x = (double)alpha_spatial / n_x, A.ws_y = (double)alpha_spatial / n_y;
  A.wt_x = (double)alpha_tv / n_x, A.wt_y = (double)alpha_tv / n_y;
  A.alpha_grad = alpha_grad;
  double* partial = (double*)workspace;
  if (big)
    L4D_LAUNCH(pg_sweep_kernel<true>, dim3(blocks), dim3(PG_THREADS), 0, stream, A, partial, g_pred_out);
  else
    L4D_LAUNCH(pg_sweep_kernel<false>, dim3(blocks), dim3(PG_THREADS), 0, stream, A, partial, g_pred_out);
  L4D_LAUNCH(pg_finish_kernel, dim3(1), dim3(PG_THREADS), 0, stream, (const double*)partial, blocks, loss_out);
  L4D_LAUNCH_CHECK("l4dg_patch_fwd");
  return 0;
}

extern "C" int l4dg_patch_bwd(const float* g_pred, const float* g, int64_t n, float* d_pred_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 1) L4D_FAIL("l4dg_patch_bwd: n must be at least 1");
  if (!g_pred || !g || !d_pred_out) L4D_FAIL("l4dg_patch_bwd: null pointer");
  const int64_t b = ceil_div64(n, PG_THREADS);
  L4D_LAUNCH(pg_scale_kernel, dim3((unsigned)(b < PG_MAX_BLOCKS ? b : PG_MAX_BLOCKS)), dim3(PG_THREADS), 0, stream, g_pred, g, n, d_pred_out);
  L4D_LAUNCH_CHECK("l4dg_patch_bwd");
  return 0;
}
