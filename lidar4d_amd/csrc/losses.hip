// The line-of-sight loss of --urf_loss (include/lidar4d_loss.h, liblidar4d_loss.so): what the reference evaluates with about
// twenty element-wise torch launches and a dozen [N,T] temporaries over the compositing weights and the sample depths
// (model/runner.py:255-276), as a value and a gradient entry point without a host step.
//
//   pre     : the normaliser m = max over all samples of bell, and n_hit.  bell is 1 at every sample that is not near and at most
//             1 elsewhere, so a wave stops reading z_vals at the first 64-sample chunk that holds a sample which is not near --
//             in practice the first chunk of its first ray; only when EVERY sample is near is this a full sweep (and m < 1).
//   sums    : one sweep over weights and z_vals: sum((empty * w)^2) and sum((near * w - b)^2), fp64 partials per workgroup.
//   finish  : one workgroup adds the partials in a fixed order and writes the loss.
//   grad    : one sweep that reads weights and z_vals and writes every element of d_weights.
// A wavefront walks a ray's samples (coalesced, 16 bytes per lane where T % 4 == 0 and the pointers allow it), as the
// compositing kernels do; exp is evaluated for near samples only, a handful per ray.  The tolerance eps comes from the
// optimiser's iteration count ON THE DEVICE (sched[0]) or from the `step` argument, through the same fp64 arithmetic.
// Nothing is zeroed and there are no floating-point atomics: the partials live in a workspace that may arrive uninitialised,
// every slot that is read has been written by the launch before, and the same input gives the same bits.
#include <stdio.h>

#include "common.h"
#include "wave_dev.h"
#include "../../include/lidar4d_loss.h"

extern "C" int l4dl_version(void) { return L4DL_ABI_VERSION; }
extern "C" const char* l4dl_last_error(void) { return l4d_last_error(); }

#define LL_THREADS 256
#define LL_WAVES (LL_THREADS / L4D_WAVE)  // rays a workgroup works on at a time: one per wavefront
#define LL_MAX_BLOCKS 2048                // the grid, and so the number of partials, is bounded; waves stride over the rays

// Workspace layout (bytes, every part 8-byte aligned)
struct LosWs {
  double* part_empty;  // [LL_MAX_BLOCKS]
  double* part_near;   // [LL_MAX_BLOCKS]
  float* part_max;     // [LL_MAX_BLOCKS]
  uint32_t* part_hit;  // [LL_MAX_BLOCKS]
};
static inline int64_t los_ws_carve(void* base, LosWs* ws) {
  char* p = (char*)base;
  int64_t off = 0;
  LosWs w;
  w.part_empty = (double*)(p + off); off += LL_MAX_BLOCKS * 8;
  w.part_near = (double*)(p + off);  off += LL_MAX_BLOCKS * 8;
  w.part_max = (float*)(p + off);    off += LL_MAX_BLOCKS * 4;
  w.part_hit = (uint32_t*)(p + off); off += LL_MAX_BLOCKS * 4;
  if (ws) *ws = w;
  return off;
}

// ---- the tolerance and a ray's bounds ------------------------------------------------------------------------------------------------
struct LosTol {
  float eps;       // (float)eps
  float two_var;   // (float)(2 sigma^2), sigma = eps / 3
};
// eps = 0.02 * 0.1 ** min(it / iters, 1) as python evaluates it (fp64); every thread of every launch takes the same route
__device__ __forceinline__ LosTol los_tolerance(const float* __restrict__ sched, int step, int iters) {
  const double it = sched ? (double)sched[0] : (double)step;
  const double frac = it / (double)iters;
  const double eps = 0.02 * pow(0.1, frac < 1.0 ? frac : 1.0);
  const double sigma = eps / 3.0;
  LosTol t;
  t.eps = (float)eps;
  t.two_var = (float)(2.0 * (sigma * sigma));
  return t;
}

struct LosRay {
  float d, lo, hi;
};
// torch's `d - eps` / `d + eps` with a python float: fp32 arithmetic on the scalar rounded to fp32; a half tensor computes in
// fp32 and rounds the result to half, and the comparison with the fp32 z_vals widens it again
__device__ __forceinline__ LosRay los_ray(const void* __restrict__ gt, int gt_half, int64_t r, float eps) {
  LosRay b;
  if (gt_half) {
    b.d = h2f(((const half_t*)gt)[r]);
    b.lo = h2f(f2h(b.d - eps));
    b.hi = h2f(f2h(b.d + eps));
  } else {
    b.d = ((const float*)gt)[r];
    b.lo = b.d - eps;
    b.hi = b.d + eps;
  }
  return b;
}
__device__ __forceinline__ bool los_near(float z, const LosRay& b) { return z > b.lo && z < b.hi; }
__device__ __forceinline__ bool los_empty(float z, const LosRay& b) { return z < b.lo || z > b.hi; }
__device__ __forceinline__ float los_bell(float z, const LosRay& b, float two_var) {
  const float x = z - b.d;
  return expf(-(x * x) / two_var);
}

// V consecutive samples of a row: one 16-byte access where V == 4
template <int V>
struct LosVec {
  float v[V];
};
template <int V>
__device__ __forceinline__ LosVec<V> los_load(const float* __restrict__ p) {
  LosVec<V> r;
  if constexpr (V == 4) {
    const float4_t q = *(const float4_t*)p;
    r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
  } else {
    r.v[0] = p[0];
  }
  return r;
}
template <int V>
__device__ __forceinline__ void los_store(float* __restrict__ p, const LosVec<V>& r) {
  if constexpr (V == 4) {
    float4_t q;
    q.x = r.v[0], q.y = r.v[1], q.z = r.v[2], q.w = r.v[3];
    *(float4_t*)p = q;
  } else {
    p[0] = r.v[0];
  }
}

// the pre-pass's partials -> normaliser and n_hit, in every thread of the workgroup
__device__ __forceinline__ void los_pre_result(const float* __restrict__ part_max, const uint32_t* __restrict__ part_hit, int n_part,
                                               float& m, double& n_hit) {
  __shared__ float sh_max[LL_WAVES];
  __shared__ double sh_hit[LL_WAVES];
  float mm = 0.0f;
  double h = 0.0;  // (integers below 2^53: exact in any order)
  for (int i = threadIdx.x; i < n_part; i += LL_THREADS) {
    mm = fmaxf(mm, part_max[i]);
    h += (double)part_hit[i];
  }
  m = block_reduce<LL_WAVES>(mm, sh_max, RedFmax());
  n_hit = block_reduce<LL_WAVES>(h, sh_hit, RedSum());
}

// ---- pre-pass: normaliser and n_hit -------------------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(LL_THREADS) los_pre_kernel(const float* __restrict__ z_vals, const void* __restrict__ gt, int gt_half,
                                                            int N, int T, const float* __restrict__ sched, int step, int iters,
                                                            float* __restrict__ part_max, uint32_t* __restrict__ part_hit) {
  __shared__ float sh_max[LL_WAVES];
  __shared__ double sh_hit[LL_WAVES];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * LL_WAVES + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * LL_WAVES;
  const LosTol tol = los_tolerance(sched, step, iters);
  float m = 0.0f;
  bool one = false;  // (wave-uniform) a sample that is not near has been seen: bell = exp(0) = 1 there, and nothing is larger
  uint32_t hits = 0;
  for (int64_t r = wave; r < N; r += n_waves) {
    const LosRay b = los_ray(gt, gt_half, r, tol.eps);
    if (lane == 0 && b.d > 0.0f) ++hits;
    if (one) continue;
    const float* __restrict__ zr = z_vals + r * (int64_t)T;
    for (int64_t t0 = 0; t0 < T; t0 += 64 * V) {
      const int64_t t = t0 + (int64_t)lane * V;
      bool not_near = false;
      if (t < T) {  // (V == 4 only with T % 4 == 0: the whole group is inside the row)
        const LosVec<V> z = los_load<V>(zr + t);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (los_near(z.v[j], b)) m = fmaxf(m, los_bell(z.v[j], b, tol.two_var));
          else not_near = true;
        }
      }
      if (__ballot(not_near)) {
        one = true;
        break;
      }
    }
  }
  m = block_reduce<LL_WAVES>(one ? 1.0f : m, sh_max, RedFmax());
  const double h = block_reduce<LL_WAVES>((double)hits, sh_hit, RedSum());
  if (threadIdx.x == 0) {
    part_max[blockIdx.x] = m;
    part_hit[blockIdx.x] = (uint32_t)h;
  }
}

// ---- the two sums ------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(LL_THREADS) los_sums_kernel(const float* __restrict__ weights, const float* __restrict__ z_vals,
                                                             const void* __restrict__ gt, int gt_half, int N, int T,
                                                             const float* __restrict__ sched, int step, int iters,
                                                             const float* __restrict__ part_max, const uint32_t* __restrict__ part_hit,
                                                             int n_part, double* __restrict__ part_empty, double* __restrict__ part_near) {
  __shared__ double sh_sum[LL_WAVES];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * LL_WAVES + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * LL_WAVES;
  const LosTol tol = los_tolerance(sched, step, iters);
  float m;
  double n_hit;
  los_pre_result(part_max, part_hit, n_part, m, n_hit);
  double s_empty = 0.0, s_near = 0.0;
  for (int64_t r = wave; r < N; r += n_waves) {
    const LosRay b = los_ray(gt, gt_half, r, tol.eps);
    const int64_t row = r * (int64_t)T;
    for (int64_t t = (int64_t)lane * V; t < T; t += 64 * V) {
      const LosVec<V> z = los_load<V>(z_vals + row + t), w = los_load<V>(weights + row + t);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (los_near(z.v[j], b)) {
          const float v = w.v[j] - los_bell(z.v[j], b, tol.two_var) / m;
          s_near += (double)(v * v);
        } else if (los_empty(z.v[j], b)) {
          s_empty += (double)(w.v[j] * w.v[j]);
        }
      }
    }
  }
  s_empty = block_reduce<LL_WAVES>(s_empty, sh_sum, RedSum());
  s_near = block_reduce<LL_WAVES>(s_near, sh_sum, RedSum());
  if (threadIdx.x == 0) {
    part_empty[blockIdx.x] = s_empty;
    part_near[blockIdx.x] = s_near;
  }
}

__global__ void __launch_bounds__(LL_THREADS) los_finish_kernel(const double* __restrict__ part_empty, const double* __restrict__ part_near,
                                                               const float* __restrict__ part_max, const uint32_t* __restrict__ part_hit,
                                                               int n_part, float* __restrict__ loss_out) {
  __shared__ double sh_sum[LL_WAVES];
  float m;
  double n_hit;
  los_pre_result(part_max, part_hit, n_part, m, n_hit);
  double s_empty = 0.0, s_near = 0.0;
  for (int i = threadIdx.x; i < n_part; i += LL_THREADS) {
    s_empty += part_empty[i];
    s_near += part_near[i];
  }
  s_empty = block_reduce<LL_WAVES>(s_empty, sh_sum, RedSum());
  s_near = block_reduce<LL_WAVES>(s_near, sh_sum, RedSum());
  if (threadIdx.x == 0) loss_out[0] = (float)(0.1 * (s_empty / n_hit) + 0.1 * (s_near / n_hit));
}

// ---- gradient ------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(LL_THREADS) los_grad_kernel(const float* __restrict__ weights, const float* __restrict__ z_vals,
                                                             const void* __restrict__ gt, int gt_half, int N, int T,
                                                             const float* __restrict__ sched, int step, int iters,
                                                             const float* __restrict__ part_max, const uint32_t* __restrict__ part_hit,
                                                             int n_part, const float* __restrict__ g, float* __restrict__ d_weights) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * LL_WAVES + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * LL_WAVES;
  const LosTol tol = los_tolerance(sched, step, iters);
  float m;
  double n_hit;
  los_pre_result(part_max, part_hit, n_part, m, n_hit);
  const float coef = (float)((double)g[0] * 0.2 / n_hit);
  for (int64_t r = wave; r < N; r += n_waves) {
    const LosRay b = los_ray(gt, gt_half, r, tol.eps);
    const int64_t row = r * (int64_t)T;
    for (int64_t t = (int64_t)lane * V; t < T; t += 64 * V) {
      const LosVec<V> z = los_load<V>(z_vals + row + t), w = los_load<V>(weights + row + t);
      LosVec<V> d;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float term = 0.0f;  // a sample exactly on a bound is neither near nor empty
        if (los_near(z.v[j], b)) term = w.v[j] - los_bell(z.v[j], b, tol.two_var) / m;
        else if (los_empty(z.v[j], b)) term = w.v[j];
        d.v[j] = coef * term;
      }
      los_store<V>(d_weights + row + t, d);
    }
  }
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
extern "C" int64_t l4dl_los_workspace(int32_t N, int32_t T) { return (N >= 1 && T >= 1) ? los_ws_carve(nullptr, nullptr) : 0; }

static inline int los_blocks(int32_t N) {
  const int64_t b = ceil_div64(N, LL_WAVES);
  return (int)(b < LL_MAX_BLOCKS ? b : LL_MAX_BLOCKS);
}
static inline bool los_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int los_check(const char* who, const void* weights, const void* z_vals, const void* gt, int32_t N, int32_t T, int32_t iters,
                     const void* out, const void* workspace) {
  static thread_local char msg[160];
  const char* what = nullptr;
  if (N < 1 || T < 1) what = "N and T must be at least 1";
  else if (iters < 1) what = "iters must be at least 1";
  else if (!weights || !z_vals || !gt || !out || !workspace) what = "null pointer";
  else if (((uintptr_t)workspace & 7) != 0) what = "workspace must be 8-byte aligned";
  if (!what) return 0;
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  l4d_set_error(1, msg);
  return 1;
}

static void los_launch_pre(bool vec, int blocks, hipStream_t stream, const float* z_vals, const void* gt, int gt_half, int N, int T,
                           const float* sched, int step, int iters, const LosWs& ws) {
  if (vec)
    L4D_LAUNCH(los_pre_kernel<4>, dim3(blocks), dim3(LL_THREADS), 0, stream, z_vals, gt, gt_half, N, T, sched, step, iters, ws.part_max,
               ws.part_hit);
  else
    L4D_LAUNCH(los_pre_kernel<1>, dim3(blocks), dim3(LL_THREADS), 0, stream, z_vals, gt, gt_half, N, T, sched, step, iters, ws.part_max,
               ws.part_hit);
}

extern "C" int l4dl_los_fwd(const float* weights, const float* z_vals, const void* gt_depth, int32_t gt_half, int32_t N, int32_t T,
                            const float* sched, int32_t step, int32_t iters, float* loss_out, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (los_check("l4dl_los_fwd", weights, z_vals, gt_depth, N, T, iters, loss_out, workspace)) return 1;
  LosWs ws;
  los_ws_carve(workspace, &ws);
  const int blocks = los_blocks(N), half = gt_half != 0;
  const bool vec = T % 4 == 0 && los_aligned16(weights) && los_aligned16(z_vals);
  los_launch_pre(vec, blocks, stream, z_vals, gt_depth, half, (int)N, (int)T, sched, (int)step, (int)iters, ws);
  if (vec)
    L4D_LAUNCH(los_sums_kernel<4>, dim3(blocks), dim3(LL_THREADS), 0, stream, weights, z_vals, gt_depth, half, (int)N, (int)T, sched,
               (int)step, (int)iters, (const float*)ws.part_max, (const uint32_t*)ws.part_hit, blocks, ws.part_empty, ws.part_near);
  else
    L4D_LAUNCH(los_sums_kernel<1>, dim3(blocks), dim3(LL_THREADS), 0, stream, weights, z_vals, gt_depth, half, (int)N, (int)T, sched,
               (int)step, (int)iters, (const float*)ws.part_max, (const uint32_t*)ws.part_hit, blocks, ws.part_empty, ws.part_near);
  L4D_LAUNCH(los_finish_kernel, dim3(1), dim3(LL_THREADS), 0, stream, (const double*)ws.part_empty, (const double*)ws.part_near,
             (const float*)ws.part_max, (const uint32_t*)ws.part_hit, blocks, loss_out);
  L4D_LAUNCH_CHECK("l4dl_los_fwd");
  return 0;
}

extern "C" int l4dl_los_bwd(const float* weights, const float* z_vals, const void* gt_depth, int32_t gt_half, int32_t N, int32_t T,
                            const float* sched, int32_t step, int32_t iters, const float* g, float* d_weights, void* workspace,
                            void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (los_check("l4dl_los_bwd", weights, z_vals, gt_depth, N, T, iters, d_weights, workspace)) return 1;
  if (!g) L4D_FAIL("l4dl_los_bwd: null pointer");
  LosWs ws;
  los_ws_carve(workspace, &ws);
  const int blocks = los_blocks(N), half = gt_half != 0;
  const bool vec = T % 4 == 0 && los_aligned16(weights) && los_aligned16(z_vals) && los_aligned16(d_weights);
  los_launch_pre(vec, blocks, stream, z_vals, gt_depth, half, (int)N, (int)T, sched, (int)step, (int)iters, ws);
  if (vec)
    L4D_LAUNCH(los_grad_kernel<4>, dim3(blocks), dim3(LL_THREADS), 0, stream, weights, z_vals, gt_depth, half, (int)N, (int)T, sched,
               (int)step, (int)iters, (const float*)ws.part_max, (const uint32_t*)ws.part_hit, blocks, g, d_weights);
  else
    L4D_LAUNCH(los_grad_kernel<1>, dim3(blocks), dim3(LL_THREADS), 0, stream, weights, z_vals, gt_depth, half, (int)N, (int)T, sched,
               (int)step, (int)iters, (const float*)ws.part_max, (const uint32_t*)ws.part_hit, blocks, g, d_weights);
  L4D_LAUNCH_CHECK("l4dl_los_bwd");
  return 0;
}
