// liblidar4d_march.so (include/lidar4d_march.h): the two kernels around a slab of the early-terminating ray march, for gfx950.
//
// A no-grad render with early_stop = eps walks every ray front to back in slabs of S samples (lidar4d_amd/early_stop.py).  The field
// and the networks of a slab are liblidar4d_hip.so's kernels on compact rows (live rays only); here are
//   slab_rows_kernel    the (x, y, z, t) rows of the live rays' samples of one slab: sample_rays_xt_kernel's (csrc/fused.hip) without
//                       noise, through the same two functions of render_dev.h;
//   slab_update_kernel  one wavefront per live ray: sigma and the 16-column fp16 rows from the compact buffers to their dense places,
//                       the slab's transmittance factors (composite_fwd_kernel's alpha: render_dev.h's alpha_of) multiplied in a fixed
//                       order (lane products, then a shuffle tree), retirement,
//                       zeros for the retired ray's remaining sigma, one flag per live ray;
//   slab_compact_kernel the flags to the next slab's live list, in order and without atomics (the ballot ranking of csrc/convert.hip;
//                       one workgroup: a list is at most one ray batch long and the pass is a few microseconds).
// No floating-point atomics anywhere: two calls give the same bits and the same order.
#include "common.h"
#include "render_dev.h"
#include "wave_dev.h"

#include "../../include/lidar4d_march.h"

extern "C" int l4dr_version(void) { return L4DR_ABI_VERSION; }
extern "C" const char* l4dr_last_error(void) { return l4d_last_error(); }

struct RedMul {
  template <typename T> __device__ __forceinline__ T operator()(T acc, T x) const { return acc * x; }
};

#define RM_RAYS 4       // rays (wavefronts) per workgroup of slab_update_kernel
#define RM_COMPACT 1024   // threads of slab_compact_kernel

__global__ void __launch_bounds__(256) march_init_kernel(int64_t N, float* __restrict__ trans, int32_t* __restrict__ live,
                                                         int32_t* __restrict__ n_live) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *n_live = (int32_t)N;
  if (i >= N) return;
  trans[i] = 1.0f;
  live[i] = (int32_t)i;
}

__global__ void __launch_bounds__(256) slab_rows_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                        const float* __restrict__ lin, const float* __restrict__ t,
                                                        const int32_t* __restrict__ live, int64_t n_live, int s0, int Sp, float near,
                                                        float far, float bound, float* __restrict__ xt) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_live * Sp) return;
  const int64_t i = idx / Sp;
  const int ti = s0 + (int)(idx - i * Sp);
  const int64_t ray = live[i];
  const float z = near + (far - near) * lin[ti];
  float4_t o;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = unit_coord(ray_point(rays_o[ray * 3 + k], rays_d[ray * 3 + k], z, bound), bound);
  }
  o[3] = *t;
  *reinterpret_cast<float4_t*>(xt + idx * 4) = o;
}

__global__ void __launch_bounds__(64 * RM_RAYS) slab_update_kernel(const float* __restrict__ sigma_c, const uint4* __restrict__ h_c,
                                                                   const float* __restrict__ z_vals, const int32_t* __restrict__ live,
                                                                   int64_t n_live, int T, int s0, int Sp, int last, float sample_dist,
                                                                   float density_scale, int active, float eps,
                                                                   float* __restrict__ trans, float* __restrict__ sigma_dense,
                                                                   uint4* __restrict__ h_dense, int32_t* __restrict__ retired_at,
                                                                   int32_t* __restrict__ alive) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * RM_RAYS + (threadIdx.x >> 6);
  if (i >= n_live) return;  // (wave-uniform; no barrier in this kernel)
  const int64_t ray = live[i];
  const float* sg = sigma_c + i * Sp;
  const float* zv = z_vals + ray * T;
  float* sd = sigma_dense + ray * T;
  float p = 1.0f;
  for (int k = lane; k < Sp; k += 64) {  // lane = sample: dense 256-byte loads and stores
    const int s = s0 + k;
    const float sgm = sg[k];
    sd[s] = sgm;
    const float delta = (s + 1 < T) ? (zv[s + 1] - zv[s]) : sample_dist;
    const float f = (1.0f - alpha_of(delta, sgm, density_scale, active)) + 1e-15f;
    p = k == lane ? f : p * f;
  }
  // the slab's h rows are contiguous on both sides: Sp * 32 bytes as 16-byte words
  const uint4* hs = h_c + i * Sp * 2;
  uint4* hd = h_dense + (ray * T + s0) * 2;
  for (int k = lane; k < Sp * 2; k += 64) hd[k] = hs[k];
  p = wave_reduce(p, RedMul());  // v[l] = v[l] * v[l + o], o = 32 ... 1: lane 0 holds the slab's product
  float tr = 0.0f;
  if (lane == 0) tr = trans[ray] * p;
  tr = __shfl(tr, 0, 64);
  const bool retired = tr < eps;  // (a NaN compares false: the ray goes on)
  if (lane == 0) {
    trans[ray] = tr;
    if (retired || last) retired_at[ray] = s0 + Sp;
    alive[i] = (retired || last) ? 0 : 1;
  }
  if (retired && !last)
    for (int s = s0 + Sp + lane; s < T; s += 64) sd[s] = 0.0f;
}

// alive [n] -> live_next: the entries of live whose flag is set, in order.  One workgroup walks the list in pieces of RM_COMPACT.
__global__ void __launch_bounds__(RM_COMPACT) slab_compact_kernel(const int32_t* __restrict__ live, const int32_t* __restrict__ alive,
                                                                  int64_t n, int32_t* __restrict__ live_next,
                                                                  int32_t* __restrict__ n_live_next) {
  __shared__ int wave_cnt[RM_COMPACT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;  // entries emitted by the pieces in front (the same in every thread)
  for (int64_t i0 = 0; i0 < n; i0 += RM_COMPACT) {
    const int64_t i = i0 + threadIdx.x;
    const bool keep = i < n && alive[i] != 0;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < RM_COMPACT / 64; ++w) {
      const int c = wave_cnt[w];
      if (w < wave) before += c;
      total += c;
    }
    if (keep) live_next[base + before + __popcll(b & ((1ull << lane) - 1ull))] = live[i];
    base += total;
    __syncthreads();  // (wave_cnt is rewritten by the next piece)
  }
  if (threadIdx.x == 0) *n_live_next = base;
}

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" int l4dr_march_init(int64_t N, float* trans, int32_t* live, int32_t* n_live, void* stream) {
  if (N < 0 || N > 0x7fffffffll) L4D_FAIL("l4dr_march_init: N outside 0 .. 2^31 - 1");
  if (N == 0) return 0;
  L4D_LAUNCH(march_init_kernel, dim3((unsigned)ceil_div64(N, 256)), dim3(256), 0, (hipStream_t)stream, N, trans, live, n_live);
  L4D_LAUNCH_CHECK("l4dr_march_init");
  return 0;
}

// the checks the two slab entry points share; -> S' (0: refused, the text is set)
static int slab_len(const char* where, int64_t n_live, int64_t N, int32_t T, int32_t s0, int32_t S) {
  static thread_local char msg[160];
  const char* what = nullptr;
  if (T < 1) what = "T must be at least 1";
  else if (S < 1) what = "S must be at least 1";
  else if (s0 < 0 || s0 >= T) what = "s0 outside 0 .. T - 1";
  else if (N < 0 || N > 0x7fffffffll) what = "N outside 0 .. 2^31 - 1";
  else if (n_live < 0 || n_live > N) what = "n_live outside 0 .. N";
  if (what) {
    snprintf(msg, sizeof msg, "%s: %s", where, what);
    l4d_set_error(1, msg);
    return 0;
  }
  return S < T - s0 ? S : T - s0;
}

extern "C" int l4dr_slab_rows(const float* rays_o, const float* rays_d, const float* lin, const float* t, const int32_t* live,
                              int64_t n_live, int64_t N, int32_t T, int32_t s0, int32_t S, float near, float far, float bound,
                              float* xt_out, void* stream) {
  const int Sp = slab_len("l4dr_slab_rows", n_live, N, T, s0, S);
  if (Sp == 0) return 1;
  if (N == 0 || n_live == 0) return 0;
  L4D_LAUNCH(slab_rows_kernel, dim3((unsigned)ceil_div64(n_live * Sp, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, lin, t,
             live, n_live, (int)s0, Sp, near, far, bound, xt_out);
  L4D_LAUNCH_CHECK("l4dr_slab_rows");
  return 0;
}

extern "C" int64_t l4dr_slab_update_workspace(int64_t n_live) { return (n_live > 0 ? n_live : 0) * 4 + 4; }

extern "C" int l4dr_slab_update(const float* sigma_c, const void* h_c, const float* z_vals, const int32_t* live, int64_t n_live,
                                int64_t N, int32_t T, int32_t s0, int32_t S, float sample_dist, float density_scale,
                                int32_t active_sensor, float eps, float* trans, float* sigma_dense, void* h_dense,
                                int32_t* retired_at, int32_t* live_next, int32_t* n_live_next, void* workspace, void* stream) {
  const int Sp = slab_len("l4dr_slab_update", n_live, N, T, s0, S);
  if (Sp == 0) return 1;
  if (!(eps >= 0.0f)) L4D_FAIL("l4dr_slab_update: eps must be a number >= 0");
  if (N == 0 || n_live == 0) return 0;
  int32_t* alive = (int32_t*)workspace;
  L4D_LAUNCH(slab_update_kernel, dim3((unsigned)ceil_div64(n_live, RM_RAYS)), dim3(64 * RM_RAYS), 0, (hipStream_t)stream, sigma_c,
             (const uint4*)h_c, z_vals, live, n_live, (int)T, (int)s0, Sp, (int)(s0 + Sp >= T), sample_dist, density_scale,
             (int)(active_sensor != 0), eps, trans, sigma_dense, (uint4*)h_dense, retired_at, alive);
  L4D_LAUNCH(slab_compact_kernel, dim3(1), dim3(RM_COMPACT), 0, (hipStream_t)stream, live, (const int32_t*)alive, n_live, live_next,
             n_live_next);
  L4D_LAUNCH_CHECK("l4dr_slab_update");
  return 0;
}
