// Point-cloud preparation for the scene-flow term (include/lidar4d_prep.h, liblidar4d_prep.so): the device-side parts of the
// reference's utils/misc.py:116-154 (point_removal), which runs on the CPU with numpy and open3d.
//
//   range filter / outlier filter : a predicate per point + ordered compaction without atomics, as csrc/convert.hip does it
//                                   (per-workgroup counts, then every workgroup sums the counts in front of it and ranks its own
//                                   points with a ballot scan).
//   k-nearest mean distance       : the statistic of open3d's remove_statistical_outlier, k <= 64 = the wavefront width.  One
//                                   wavefront serves KNN_Q queries; lane l holds ONE of a query's current k best squared
//                                   distances, the wave maximum is the rejection bound.  Per step every lane loads one candidate
//                                   (structure-of-arrays copy of the cloud: three coalesced 4-byte loads, shared by the KNN_Q
//                                   queries), computes d^2 and votes d^2 < bound; after warm-up the ballot is almost always empty.
//                                   An accepted candidate replaces the lane that holds the bound and the bound is reduced again
//                                   (DPP).  A thread-per-query form would keep a 64-entry list per thread in scratch.
//                                   The scan starts at the queries' own batch of 64 and goes outwards in the (caller-sorted)
//                                   order; a batch whose bounding box lies beyond the bound of every query is skipped, which
//                                   loses nothing: exact.
//   plane scoring                 : RANSAC hypotheses in batches: one thread fits each triple, then one thread per point holds the
//                                   point in registers and walks the (wave-uniform) hypotheses, ballot + popcount, LDS integer
//                                   counters, one global atomic add per workgroup and hypothesis.  Integer sums: deterministic.
// fp32 arithmetic with separate multiplies and adds (-ffp-contract=off), i.e. numpy's on a float32 cloud.
#include "common.h"
#include "wave_dev.h"
#include "../../include/lidar4d_prep.h"

extern "C" int l4dp_version(void) { return L4DP_ABI_VERSION; }
extern "C" const char* l4dp_last_error(void) { return l4d_last_error(); }

#define PP_MAX_POINTS ((int64_t)1 << 28)  // 32-bit indices and byte offsets throughout

// ---- predicates + ordered compaction ---------------------------------------------------------------------------------------------
#define PC_THREADS 1024

struct RangePred {  // utils/misc.py:116-124
  float dist_min, dist_max, z_min, z_max;
  __device__ __forceinline__ bool operator()(const float* __restrict__ pts, int64_t i) const {
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    const float dist = sqrtf(x * x + y * y + z * z);
    const bool ego = x > -2.0f && x < 2.0f && y > -1.0f && y < 1.0f && z > -2.0f && z < 2.0f;
    return dist >= dist_min && dist <= dist_max && z > z_min && z < z_max && !ego;
  }
};

struct BelowPred {  // avg[i] < stats[2], compared in fp64
  const float* avg;
  const double* stats;
  __device__ __forceinline__ bool operator()(const float* __restrict__, int64_t i) const { return (double)avg[i] < stats[2]; }
};

template <class Pred>
__global__ void __launch_bounds__(PC_THREADS) compact_count_kernel(const float* __restrict__ pts, int64_t n, Pred pred,
                                                                  int32_t* __restrict__ counts) {
  __shared__ int wave_cnt[PC_THREADS / 64];
  const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
  const bool keep = i < n && pred(pts, i);
  const unsigned long long b = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < PC_THREADS / 64; ++w) s += wave_cnt[w];
    counts[blockIdx.x] = s;
  }
}

template <class Pred>
__global__ void __launch_bounds__(PC_THREADS) compact_emit_kernel(const float* __restrict__ pts, int64_t n, Pred pred,
                                                                 const int32_t* __restrict__ counts, float* __restrict__ out,
                                                                 int32_t* __restrict__ out_index, int32_t* __restrict__ total) {
  __shared__ int wave_cnt[PC_THREADS / 64];
  __shared__ int part[PC_THREADS / 64];
  __shared__ int base_s;
  // points kept by the workgroups in front of this one
  int acc = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += PC_THREADS) acc += counts[k];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = acc;
  const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
  const bool keep = i < n && pred(pts, i);
  const unsigned long long b = __ballot(keep);
  if (lane == 0) wave_cnt[wave] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < PC_THREADS / 64; ++w) s += part[w];
    base_s = s;
    if (blockIdx.x == gridDim.x - 1) {
      int mine = 0;
      for (int w = 0; w < PC_THREADS / 64; ++w) mine += wave_cnt[w];
      *total = s + mine;
    }
  }
  __syncthreads();
  if (!keep) return;
  int pos = base_s + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
  out[(int64_t)pos * 3] = pts[i * 3];
  out[(int64_t)pos * 3 + 1] = pts[i * 3 + 1];
  out[(int64_t)pos * 3 + 2] = pts[i * 3 + 2];
  if (out_index) out_index[pos] = (int32_t)i;
}

template <class Pred>
static void compact_launch(const float* pts, int64_t n, Pred pred, float* out, int32_t* out_index, int32_t* count, void* workspace,
                           hipStream_t stream) {
  const unsigned blocks = (unsigned)ceil_div64(n, PC_THREADS);
  int32_t* counts = (int32_t*)workspace;
  L4D_LAUNCH(compact_count_kernel<Pred>, dim3(blocks), dim3(PC_THREADS), 0, stream, pts, n, pred, counts);
  L4D_LAUNCH(compact_emit_kernel<Pred>, dim3(blocks), dim3(PC_THREADS), 0, stream, pts, n, pred, (const int32_t*)counts, out,
             out_index, count);
}

extern "C" int64_t l4dp_compact_workspace(int64_t n) { return (ceil_div64(n > 0 ? n : 0, PC_THREADS) + 1) * 4; }

extern "C" int l4dp_range_filter(const float* points, int64_t n, float dist_min, float dist_max, float z_min, float z_max,
                                 float* out, int32_t* out_index, int32_t* count, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || n > PP_MAX_POINTS || !count) L4D_FAIL("l4dp_range_filter: bad n or null count");
  if (n == 0) { l4d_fill_async(count, 0u, 4, stream); return 0; }
  if (!points || !out || !workspace) L4D_FAIL("l4dp_range_filter: null pointer");
  RangePred pred{dist_min, dist_max, z_min, z_max};
  compact_launch(points, n, pred, out, out_index, count, workspace, stream);
  L4D_LAUNCH_CHECK("l4dp_range_filter");
  return 0;
}

// ---- k-nearest mean distance -------------------------------------------------------------------------------------------------
#define KNN_Q 4      // queries per wavefront (share every candidate load)
#define KNN_WAVES 4  // wavefronts per workgroup

// Workspace: the cloud in visiting order as structure of arrays, padded to whole batches of 64 with +inf (d^2 = inf is never
// accepted), then the bounding box of every batch (6 arrays: lo x/y/z, hi x/y/z), padded to whole groups of 64 batches with an
// empty box (lo = +inf, hi = -inf: its distance to anything is inf).  One wavefront per batch.
__global__ void __launch_bounds__(256) knn_soa_kernel(const float* __restrict__ pts, const int32_t* __restrict__ order, int n, int n_pad,
                                                      int nb_pad, float* __restrict__ soa, float* __restrict__ box) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // < nb_pad * 64 (the grid is exact)
  const float inf = __builtin_inff();
  float x = inf, y = inf, z = inf;
  if (i < n) {
    int src = order ? order[i] : i;
    src = min(max(src, 0), n - 1);  // (a permutation by contract; never read out of bounds if it is not)
    x = pts[(int64_t)src * 3];
    y = pts[(int64_t)src * 3 + 1];
    z = pts[(int64_t)src * 3 + 2];
  }
  if (i < n_pad) {
    soa[i] = x;
    soa[n_pad + i] = y;
    soa[2 * n_pad + i] = z;
  }
  float lo[3] = {x, y, z}, hi[3] = {x, y, z};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (i >= n) hi[d] = -inf;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[d] = fminf(lo[d], __shfl_xor(lo[d], o));
      hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o));
    }
  }
  if ((threadIdx.x & 63) == 0) {
    const int b = i >> 6;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      box[d * nb_pad + b] = lo[d];
      box[(3 + d) * nb_pad + b] = hi[d];
    }
  }
}

__device__ __forceinline__ float knn_readlane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// Wave maximum of non-negative floats (+inf included) as a wave-uniform value, on their BIT PATTERNS: they order like unsigned
// integers, and 0 -- what a DPP step reads where it has no source lane -- is the identity of an unsigned maximum, so each of the six
// steps of wave_dev.h's wave_max folds into one v_max_u32_dpp (the float form keeps a move and two canonicalising v_max_f32 per
// step).  This reduction follows every accepted candidate and is most of what an insertion costs.
__device__ __forceinline__ float knn_wave_max(float f) {
  unsigned v = __float_as_uint(f);
#define KNN_MAX_DPP(ctrl, rmask) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xf, false))
  KNN_MAX_DPP(0x111, 0xf);  // row_shr:1
  KNN_MAX_DPP(0x112, 0xf);  // row_shr:2
  KNN_MAX_DPP(0x114, 0xf);  // row_shr:4
  KNN_MAX_DPP(0x118, 0xf);  // row_shr:8   -> lane 15 of each row holds the row maximum
  KNN_MAX_DPP(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
  KNN_MAX_DPP(0x143, 0xc);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave maximum
#undef KNN_MAX_DPP
  return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)v, 63));
}

// the set bit of m (non-zero) nearest to position p; p = -1: the lowest, p = 64: the highest
__device__ __forceinline__ int knn_pick_near(unsigned long long m, int p) {
  const unsigned long long above = p >= 63 ? 0ull : (p < 0 ? m : m & (~0ull << (p + 1)));
  const unsigned long long below = p <= 0 ? 0ull : (p > 63 ? m : m & ((1ull << p) - 1ull));
  const int up = above ? __ffsll((long long)above) - 1 : 1 << 20;
  const int down = below ? 63 - __clzll((long long)below) : -(1 << 20);
  return up - p <= p - down ? up : down;
}

// The scan is two-level.  Batches are visited in groups of 64: lane l takes the box of the group's batch l and votes whether that
// batch can still hold a point closer than the bound of ANY of the wavefront's queries (squared distance from the query to the box:
// computed with the same roundings as a candidate's d^2 and never larger than it, so a batch that is voted out holds nothing that
// would have been accepted -- the result stays exact); only the batches voted in are loaded.  In Morton order a batch is a compact
// blob and all but a few dozen of a frame's ~1000 batches are voted out; in input order the boxes cover the scene, every batch
// is visited, and the vote costs 1/64 of a step.
__global__ void __launch_bounds__(KNN_WAVES * 64) knn_mean_dist_kernel(const float* __restrict__ soa, const float* __restrict__ box,
                                                                      int n, int n_pad, int nb_pad, int k_eff,
                                                                      const int32_t* __restrict__ order, float* __restrict__ avg) {
  const int lane = threadIdx.x & 63;
  const int q0 = (blockIdx.x * KNN_WAVES + (threadIdx.x >> 6)) * KNN_Q;  // wave-uniform
  if (q0 >= n) return;
  const float* __restrict__ xs = soa;
  const float* __restrict__ ys = soa + n_pad;
  const float* __restrict__ zs = soa + 2 * n_pad;
  const float inf = __builtin_inff();
  float qx[KNN_Q], qy[KNN_Q], qz[KNN_Q], best[KNN_Q], bound[KNN_Q];
#pragma unroll
  for (int q = 0; q < KNN_Q; ++q) {
    const int qi = min(q0 + q, n - 1);  // (a short last group repeats its last query)
    qx[q] = xs[qi];
    qy[q] = ys[qi];
    qz[q] = zs[qi];
    best[q] = lane < k_eff ? inf : 0.0f;  // lanes >= k_eff hold 0: neutral for the maximum, left out of the sum
    bound[q] = inf;
  }
  // one batch of 64 candidates against the KNN_Q queries
  auto visit = [&](int b, bool take_whole) {
    const int j = (b << 6) + lane;
    const float cx = xs[j], cy = ys[j], cz = zs[j];
#pragma unroll
    for (int q = 0; q < KNN_Q; ++q) {
      const float dx = cx - qx[q], dy = cy - qy[q], dz = cz - qz[q];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (take_whole) {  // first batch, all 64 lanes free and 64 real candidates
        best[q] = d2;
        bound[q] = knn_wave_max(d2);
        continue;
      }
      unsigned long long m = __ballot(d2 < bound[q]);
      while (m) {  // wave-uniform; rare once the bound has settled
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float dj = knn_readlane(d2, src);
        if (dj < bound[q]) {  // (the bound may have dropped since the vote)
          const unsigned long long holders = __ballot(best[q] == bound[q] && lane < k_eff);
          if (lane == __ffsll((long long)holders) - 1) best[q] = dj;
          bound[q] = knn_wave_max(best[q]);
        }
      }
    }
  };
  // the queries' own batch first: in Morton order it holds most of their neighbours, and the bound is close to final after it
  const int c = q0 >> 6;
  visit(c, k_eff == 64 && (c << 6) + 64 <= n);
  const int ng = nb_pad >> 6, cg = c >> 6;
  const int span = max(cg, ng - 1 - cg);
  for (int s = 0; s <= 2 * span; ++s) {  // groups cg, cg+1, cg-1, cg+2, cg-2, ...
    const int off = (s + 1) >> 1;
    const int g = (s & 1) ? cg + off : cg - off;
    if (g < 0 || g >= ng) continue;
    const int bl = (g << 6) + lane;
    const float lox = box[bl], loy = box[nb_pad + bl], loz = box[2 * nb_pad + bl];
    const float hix = box[3 * nb_pad + bl], hiy = box[4 * nb_pad + bl], hiz = box[5 * nb_pad + bl];
    float e2[KNN_Q];  // squared distance from query q to the box of this lane's batch
#pragma unroll
    for (int q = 0; q < KNN_Q; ++q) {
      const float ex = fmaxf(fmaxf(lox - qx[q], qx[q] - hix), 0.0f);
      const float ey = fmaxf(fmaxf(loy - qy[q], qy[q] - hiy), 0.0f);
      const float ez = fmaxf(fmaxf(loz - qz[q], qz[q] - hiz), 0.0f);
      e2[q] = ex * ex + ey * ey + ez * ez;
    }
    // nearest batches first (own group: outwards from the own batch; groups above: ascending; below: descending), and the vote is
    // taken again after every visit: each visit can lower the bounds and vote more batches out
    const int near = g == cg ? (c & 63) : (g > cg ? -1 : 64);
    unsigned long long remaining = g == cg ? ~(1ull << (c & 63)) : ~0ull;
    for (;;) {
      bool need = false;
#pragma unroll
      for (int q = 0; q < KNN_Q; ++q) need = need || e2[q] < bound[q];
      const unsigned long long todo = __ballot(need) & remaining;
      if (!todo) break;
      const int pick = knn_pick_near(todo, near);
      remaining &= ~(1ull << pick);
      visit((g << 6) + pick, false);
    }
  }
#pragma unroll
  for (int q = 0; q < KNN_Q; ++q) {
    float v = lane < k_eff ? sqrtf(best[q]) : 0.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);  // fixed tree: the same sum on every run
    const int qi = q0 + q;
    if (lane == 0 && qi < n) {
      int dst = order ? order[qi] : qi;
      dst = min(max(dst, 0), n - 1);
      avg[dst] = v / (float)k_eff;
    }
  }
}

static inline int64_t knn_pad(int64_t n) { return ceil_div64(n, 64) * 64; }
static inline int64_t knn_box_pad(int64_t n) { return ceil_div64(knn_pad(n) / 64, 64) * 64; }

extern "C" int64_t l4dp_knn_workspace(int64_t n) { return n > 0 ? (knn_pad(n) * 3 + knn_box_pad(n) * 6) * 4 : 4; }

extern "C" int l4dp_knn_mean_dist(const float* points, int64_t n, int32_t k, const int32_t* order, float* avg, void* workspace,
                                  void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || n > PP_MAX_POINTS) L4D_FAIL("l4dp_knn_mean_dist: bad n");
  if (k < 1 || k > L4DP_MAX_NEIGHBORS) L4D_FAIL("l4dp_knn_mean_dist: k must be in [1, 64]");
  if (n == 0) return 0;
  if (!points || !avg || !workspace) L4D_FAIL("l4dp_knn_mean_dist: null pointer");
  const int n_pad = (int)knn_pad(n), nb_pad = (int)knn_box_pad(n);
  const int k_eff = (int)(k < n ? k : n);
  float* soa = (float*)workspace;
  float* box = soa + (size_t)3 * n_pad;
  L4D_LAUNCH(knn_soa_kernel, dim3((unsigned)(nb_pad / 4)), dim3(256), 0, stream, points, order, (int)n, n_pad, nb_pad, soa, box);
  const unsigned blocks = (unsigned)ceil_div64(n, KNN_Q * KNN_WAVES);
  L4D_LAUNCH(knn_mean_dist_kernel, dim3(blocks), dim3(KNN_WAVES * 64), 0, stream, (const float*)soa, (const float*)box, (int)n, n_pad,
             nb_pad, k_eff, order, avg);
  L4D_LAUNCH_CHECK("l4dp_knn_mean_dist");
  return 0;
}

// ---- outlier threshold -----------------------------------------------------------------------------------------------------------
#define ST_THREADS 1024

// sum over the workgroup in a fixed order (the same value in every thread).  Not wave_dev.h's block_reduce: the xor butterfly
// needs no per-step lane select, which the down-tree pays for with six more registers in this kernel.
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // (sh may still be read from the call before)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < ST_THREADS / 64; ++w) s += sh[w];
  return s;
}

// one workgroup: n <= 131,072 values are 128 per thread, and a single fixed reduction tree keeps mu and sd reproducible
__global__ void __launch_bounds__(ST_THREADS) outlier_stats_kernel(const float* __restrict__ avg, int64_t n, double std_ratio,
                                                                  double* __restrict__ stats) {
  __shared__ double sh[ST_THREADS / 64];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += ST_THREADS) s += (double)avg[i];
  const double mu = block_sum_f64(s, sh) / (double)n;
  double ss = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += ST_THREADS) {
    const double d = (double)avg[i] - mu;
    ss += d * d;
  }
  const double sd = sqrt(block_sum_f64(ss, sh) / (double)(n - 1));
  if (threadIdx.x == 0) {
    stats[0] = mu;
    stats[1] = sd;
    stats[2] = mu + std_ratio * sd;
  }
}

extern "C" int l4dp_outlier_filter(const float* points, const float* avg, int64_t n, double std_ratio, float* out,
                                   int32_t* out_index, int32_t* count, double* stats, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || n > PP_MAX_POINTS || !count) L4D_FAIL("l4dp_outlier_filter: bad n or null count");
  if (n == 0) { l4d_fill_async(count, 0u, 4, stream); return 0; }
  if (!points || !avg || !out || !stats || !workspace) L4D_FAIL("l4dp_outlier_filter: null pointer");
  L4D_LAUNCH(outlier_stats_kernel, dim3(1), dim3(ST_THREADS), 0, stream, avg, n, std_ratio, stats);
  BelowPred pred{avg, stats};
  compact_launch(points, n, pred, out, out_index, count, workspace, stream);
  L4D_LAUNCH_CHECK("l4dp_outlier_filter");
  return 0;
}

// ---- RANSAC plane hypotheses -------------------------------------------------------------------------------------------------
#define PL_THREADS 256
#define PL_CHUNK 256  // hypotheses per pass over the LDS counters

// utils/misc.py:83-87 (the y-gap redraw) and 18-57 (estimate_plane, normalize=False)
__global__ void plane_fit_kernel(const float* __restrict__ pts, int n, const int32_t* __restrict__ triples, int n_hyp, float y_gap,
                                 int32_t* __restrict__ valid, float* __restrict__ coeffs, int32_t* __restrict__ counts) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_hyp) return;
  const int i0 = triples[h * 3], i1 = triples[h * 3 + 1], i2 = triples[h * 3 + 2];
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
  bool ok = i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n;
  if (ok) {
    const float x0 = pts[(int64_t)i0 * 3], y0 = pts[(int64_t)i0 * 3 + 1], z0 = pts[(int64_t)i0 * 3 + 2];
    const float y1 = pts[(int64_t)i1 * 3 + 1];
    const float v1x = pts[(int64_t)i1 * 3] - x0, v1y = y1 - y0, v1z = pts[(int64_t)i1 * 3 + 2] - z0;
    const float v2x = pts[(int64_t)i2 * 3] - x0, v2y = pts[(int64_t)i2 * 3 + 1] - y0, v2z = pts[(int64_t)i2 * 3 + 2] - z0;
    ok = !(fabsf(y0 - y1) < y_gap) && v1x != 0.0f && v1y != 0.0f && v1z != 0.0f;
    if (ok) {
      const float rx = v2x / v1x, ry = v2y / v1y, rz = v2z / v1z;
      ok = rx != ry || rz != ry;
    }
    if (ok) {
      a = v1y * v2z - v1z * v2y;
      b = v1z * v2x - v1x * v2z;
      c = v1x * v2y - v1y * v2x;
      d = -(a * x0 + b * y0 + c * z0);
    }
  }
  valid[h] = ok ? 1 : 0;
  coeffs[h * 4] = a;
  coeffs[h * 4 + 1] = b;
  coeffs[h * 4 + 2] = c;
  coeffs[h * 4 + 3] = d;
  counts[h] = 0;
}

// utils/misc.py:90-91: |n . p + d| / |n| < threshold
__device__ __forceinline__ bool plane_near(const float* __restrict__ co, float x, float y, float z, float threshold) {
  const float a = co[0], b = co[1], c = co[2], d = co[3];
  const float r = sqrtf(a * a + b * b + c * c);
  return fabsf(a * x + b * y + c * z + d) / r < threshold;
}

__global__ void __launch_bounds__(PL_THREADS) plane_count_kernel(const float* __restrict__ pts, int n, const int32_t* __restrict__ valid,
                                                                const float* __restrict__ coeffs, int n_hyp, float threshold,
                                                                int32_t* __restrict__ counts) {
  __shared__ int cnt[PL_CHUNK];
  const int i = blockIdx.x * PL_THREADS + threadIdx.x;
  const bool live = i < n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) { x = pts[(int64_t)i * 3]; y = pts[(int64_t)i * 3 + 1]; z = pts[(int64_t)i * 3 + 2]; }
  for (int h0 = 0; h0 < n_hyp; h0 += PL_CHUNK) {
    const int hn = min(PL_CHUNK, n_hyp - h0);
    __syncthreads();
    if ((int)threadIdx.x < hn) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int h = 0; h < hn; ++h) {
      if (!valid[h0 + h]) continue;  // wave-uniform
      const unsigned long long b = __ballot(live && plane_near(coeffs + (int64_t)(h0 + h) * 4, x, y, z, threshold));
      if ((threadIdx.x & 63) == 0 && b) atomicAdd(&cnt[h], __popcll(b));
    }
    __syncthreads();
    if ((int)threadIdx.x < hn && cnt[threadIdx.x]) atomicAdd(counts + h0 + threadIdx.x, cnt[threadIdx.x]);
  }
}

__global__ void __launch_bounds__(PL_THREADS) plane_mask_kernel(const float* __restrict__ pts, int n, const float* __restrict__ coeffs,
                                                               int n_planes, float threshold, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * PL_THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = pts[(int64_t)i * 3], y = pts[(int64_t)i * 3 + 1], z = pts[(int64_t)i * 3 + 2];
  bool near = false;
  for (int h = 0; h < n_planes; ++h) near = near || plane_near(coeffs + (int64_t)h * 4, x, y, z, threshold);
  if (near) mask[i] |= 1;  // (the header's contract: the other bits of the byte are the caller's)
}

extern "C" int l4dp_plane_score(const float* points, int64_t n, const int32_t* triples, int32_t n_hyp, float y_gap, float threshold,
                                int32_t* valid, float* coeffs, int32_t* counts, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || n > PP_MAX_POINTS || n_hyp < 0) L4D_FAIL("l4dp_plane_score: bad n or n_hyp");
  if (n_hyp == 0) return 0;
  if (!triples || !valid || !coeffs || !counts || (n > 0 && !points)) L4D_FAIL("l4dp_plane_score: null pointer");
  L4D_LAUNCH(plane_fit_kernel, dim3((unsigned)ceil_div64(n_hyp, 64)), dim3(64), 0, stream, points, (int)n, triples, (int)n_hyp, y_gap,
             valid, coeffs, counts);
  if (n > 0)
    L4D_LAUNCH(plane_count_kernel, dim3((unsigned)ceil_div64(n, PL_THREADS)), dim3(PL_THREADS), 0, stream, points, (int)n,
               (const int32_t*)valid, (const float*)coeffs, (int)n_hyp, threshold, counts);
  L4D_LAUNCH_CHECK("l4dp_plane_score");
  return 0;
}

extern "C" int l4dp_plane_mask(const float* points, int64_t n, const float* coeffs, int32_t n_planes, float threshold, uint8_t* mask,
                               void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || n > PP_MAX_POINTS || n_planes < 0) L4D_FAIL("l4dp_plane_mask: bad n or n_planes");
  if (n == 0 || n_planes == 0) return 0;
  if (!points || !coeffs || !mask) L4D_FAIL("l4dp_plane_mask: null pointer");
  L4D_LAUNCH(plane_mask_kernel, dim3((unsigned)ceil_div64(n, PL_THREADS)), dim3(PL_THREADS), 0, stream, points, (int)n, coeffs,
             (int)n_planes, threshold, mask);
  L4D_LAUNCH_CHECK("l4dp_plane_mask");
  return 0;
}
