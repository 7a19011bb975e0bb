// Error statistics of a rendered image against the ground truth (include/lidar4d_eval.h, liblidar4d_eval.so): what the
// reference's DepthMeter / IntensityMeter compute with numpy and skimage on the host (utils/metrics.py:64-86,135-157), as one
// sync-free entry point.  The frame is small (66 x 1030); the point is few launches and no host step, not bandwidth.
//
//   fill        : zeroes the radix-select histograms (a kernel, common.h: no memset node).
//   errors      : clamp, d = g - p, |d| kept as its bit pattern, sum of d^2 (fp64) and min / max of g as per-workgroup partials,
//                 histogram of the top byte of |d|.
//   ssim        : one workgroup per 16 x 32 tile of windows: the clamped tile with its 6-pixel apron in LDS, 7-tap row sums of
//                 p, g, pp, gg, pg into LDS, 7-tap column sums, S per window, one partial per workgroup.  fp64 after the clamp:
//                 uxx - ux*ux at depths up to 80 cancels too much for fp32.
//   select x 3  : radix select, 8 bits per pass, for the two middle order statistics at once.  Non-negative floats order like
//                 their bit patterns.  Every workgroup re-derives the prefixes chosen so far from the (complete) histograms of
//                 the earlier passes -- no state besides the histograms -- and counts the next byte of the keys under each
//                 prefix.  LDS integer counters, one global integer atomic per non-empty bin and workgroup.
//   finalise    : sums the partials, resolves the last byte, writes rmse / medae / ssim / psnr.
// Every floating-point reduction has a fixed order (thread-strided sums, shuffle tree, waves in order; partials summed by one
// workgroup); the only atomics are integer counters.  The same input gives the same bits.
#include "common.h"
#include "wave_dev.h"
#include "../../include/lidar4d_eval.h"

extern "C" int l4de_version(void) { return L4DE_ABI_VERSION; }
extern "C" const char* l4de_last_error(void) { return l4d_last_error(); }

#define EM_THREADS 256
#define EM_WAVES (EM_THREADS / L4D_WAVE)
#define EM_CHUNK 2048          // pixels per workgroup and grid-stride step of the streaming kernels
#define EM_MAX_BLOCKS 1024     // ... whose grid, and so the number of partials, is bounded
#define EM_MAX_PIXELS ((int64_t)1 << 28)
#define EM_PASSES 4            // 8 bits of the 32-bit key per pass
#define SS_WIN L4DE_SSIM_WINDOW
#define SS_TH 16               // windows per tile
#define SS_TW 32
#define SS_IH (SS_TH + SS_WIN - 1)
#define SS_IW (SS_TW + SS_WIN - 1)

// Workspace layout (bytes, every part 8-byte aligned)
struct EvalWs {
  uint32_t* hist;    // [EM_PASSES][2][256]: pass, rank (lower / upper middle), digit; pass 0 uses rank 0 only
  double* part_sq;   // [EM_MAX_BLOCKS]
  float* part_min;   // [EM_MAX_BLOCKS]
  float* part_max;   // [EM_MAX_BLOCKS]
  double* part_ssim; // [tiles]
  uint32_t* absd;    // [n]
};
static inline int64_t ssim_tiles(int32_t H, int32_t W) {
  return ceil_div64(H - (SS_WIN - 1), SS_TH) * ceil_div64(W - (SS_WIN - 1), SS_TW);
}
static inline int64_t eval_ws_carve(void* base, int32_t H, int32_t W, EvalWs* ws) {
  char* p = (char*)base;
  int64_t off = 0;
  EvalWs w;
  w.hist = (uint32_t*)(p + off);   off += EM_PASSES * 2 * 256 * 4;
  w.part_sq = (double*)(p + off);  off += EM_MAX_BLOCKS * 8;
  w.part_min = (float*)(p + off);  off += EM_MAX_BLOCKS * 4;
  w.part_max = (float*)(p + off);  off += EM_MAX_BLOCKS * 4;
  w.part_ssim = (double*)(p + off); off += ssim_tiles(H, W) * 8;
  w.absd = (uint32_t*)(p + off);   off += ceil_div64((int64_t)H * W, 2) * 8;
  if (ws) *ws = w;
  return off;
}
static inline bool eval_shape_ok(int32_t H, int32_t W) {
  return H >= SS_WIN && W >= SS_WIN && (int64_t)H * W <= EM_MAX_PIXELS;
}

// the reference's masked assignments (x[x < lo] = lo; x[x > hi] = hi): a NaN fails both comparisons and stays
__device__ __forceinline__ float clamp_keep_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ---- pass over the pixels: differences, partial sums, first histogram ---------------------------------------------------------------
__global__ void __launch_bounds__(EM_THREADS) eval_errors_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n,
                                                                float lo, float hi, uint32_t* __restrict__ absd,
                                                                uint32_t* __restrict__ hist0, double* __restrict__ part_sq,
                                                                float* __restrict__ part_min, float* __restrict__ part_max) {
  __shared__ uint32_t bins[256];
  __shared__ double sh_sum[EM_WAVES];
  __shared__ float sh_min[EM_WAVES], sh_max[EM_WAVES];
  const int t = threadIdx.x;
  bins[t] = 0;
  __syncthreads();
  double sq = 0.0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int64_t base = (int64_t)blockIdx.x * EM_CHUNK; base < n; base += (int64_t)gridDim.x * EM_CHUNK) {
#pragma unroll
    for (int j = 0; j < EM_CHUNK / EM_THREADS; ++j) {
      const int64_t i = base + j * EM_THREADS + t;
      if (i >= n) break;
      const float p = clamp_keep_nan(pred[i], lo, hi), g = clamp_keep_nan(gt[i], lo, hi);
      const float d = g - p;
      const uint32_t key = __float_as_uint(fabsf(d));
      absd[i] = key;
      sq += (double)d * (double)d;
      mn = g < mn ? g : mn;
      mx = g > mx ? g : mx;
      atomicAdd(&bins[key >> 24], 1u);
    }
  }
  mn = wave_reduce(mn, RedMin());
  mx = wave_reduce(mx, RedMax());
  if ((t & 63) == 0) { sh_min[t >> 6] = mn; sh_max[t >> 6] = mx; }
  sq = block_reduce<EM_WAVES>(sq, sh_sum, RedSum());  // (its barriers also cover sh_min / sh_max and bins)
  if (t == 0) {
    part_min[blockIdx.x] = waves_combine<EM_WAVES>(sh_min, RedMin());
    part_max[blockIdx.x] = waves_combine<EM_WAVES>(sh_max, RedMax());
    part_sq[blockIdx.x] = sq;
  }
  if (bins[t]) atomicAdd(&hist0[t], bins[t]);
}

// ---- radix select ---------------------------------------------------------------------------------------------------------------
// One wavefront, all 64 lanes: the digit whose bin holds rank k of a 256-bin histogram, and k reduced to the rank inside that bin.
__device__ __forceinline__ uint32_t pick_digit(const uint32_t* __restrict__ hist, uint32_t& k) {
  const int lane = threadIdx.x & 63;
  const uint32_t h0 = hist[lane * 4], h1 = hist[lane * 4 + 1], h2 = hist[lane * 4 + 2], h3 = hist[lane * 4 + 3];
  const uint32_t own = h0 + h1 + h2 + h3;
  uint32_t inc = own;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  const uint32_t exc = inc - own;
  const unsigned long long hit = __ballot(k >= exc && k < inc);
  const int src = hit ? __ffsll((long long)hit) - 1 : 63;  // (k < total always: hit is never empty)
  uint32_t kk = k - exc, sub = 0;
  if (kk >= h0) { kk -= h0; sub = 1; if (kk >= h1) { kk -= h1; sub = 2; if (kk >= h2) { kk -= h2; sub = 3; } } }
  k = __shfl(kk, src);
  return __shfl((uint32_t)lane * 4 + sub, src);
}

// The key prefix (passes 0 .. n_pass-1, 8 bits each) under which rank k of all keys lies, and k inside it.  rank_slot: 0 / 1.
__device__ __forceinline__ uint32_t select_prefix(const uint32_t* __restrict__ hist, int n_pass, int rank_slot, uint32_t& k) {
  uint32_t prefix = 0;
  for (int q = 0; q < n_pass; ++q) prefix = (prefix << 8) | pick_digit(hist + (q * 2 + (q == 0 ? 0 : rank_slot)) * 256, k);
  return prefix;
}

__global__ void __launch_bounds__(EM_THREADS) eval_select_kernel(const uint32_t* __restrict__ absd, int n, int pass,
                                                                uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[2][256];
  __shared__ uint32_t sh_prefix[2];
  const int t = threadIdx.x;
  bins[0][t] = 0;
  bins[1][t] = 0;
  if (t < 64) {
    uint32_t k0 = (uint32_t)(n - 1) >> 1, k1 = (uint32_t)n >> 1;
    const uint32_t p0 = select_prefix(hist, pass, 0, k0), p1 = select_prefix(hist, pass, 1, k1);
    if (t == 0) { sh_prefix[0] = p0; sh_prefix[1] = p1; }
  }
  __syncthreads();
  const uint32_t p0 = sh_prefix[0], p1 = sh_prefix[1];
  const int hi_shift = 32 - 8 * pass, lo_shift = 24 - 8 * pass;
  for (int64_t base = (int64_t)blockIdx.x * EM_CHUNK; base < n; base += (int64_t)gridDim.x * EM_CHUNK) {
#pragma unroll
    for (int j = 0; j < EM_CHUNK / EM_THREADS; ++j) {
      const int64_t i = base + j * EM_THREADS + t;
      if (i >= n) break;
      const uint32_t key = absd[i], head = key >> hi_shift, digit = (key >> lo_shift) & 255u;
      if (head == p0) atomicAdd(&bins[0][digit], 1u);
      if (head == p1) atomicAdd(&bins[1][digit], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = hist + pass * 2 * 256;
  if (bins[0][t]) atomicAdd(&out[t], bins[0][t]);
  if (bins[1][t]) atomicAdd(&out[256 + t], bins[1][t]);
}

// ---- SSIM ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EM_THREADS) eval_ssim_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                              float lo, float hi, const float* __restrict__ part_min,
                                                              const float* __restrict__ part_max, int n_part, int tiles_x,
                                                              double* __restrict__ part_ssim) {
  __shared__ float sp[SS_IH][SS_IW], sg[SS_IH][SS_IW];
  __shared__ double rows[5][SS_IH][SS_TW];
  __shared__ double sh_sum[EM_WAVES];
  __shared__ float sh_min[EM_WAVES], sh_max[EM_WAVES];
  const int t = threadIdx.x;
  const int y0 = (int)(blockIdx.x / tiles_x) * SS_TH, x0 = (int)(blockIdx.x % tiles_x) * SS_TW;
  // data range of the clamped ground truth from the first pass's partials
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = t; i < n_part; i += EM_THREADS) {
    mn = part_min[i] < mn ? part_min[i] : mn;
    mx = part_max[i] > mx ? part_max[i] : mx;
  }
  mn = wave_reduce(mn, RedMin());
  mx = wave_reduce(mx, RedMax());
  if ((t & 63) == 0) { sh_min[t >> 6] = mn; sh_max[t >> 6] = mx; }
  // the clamped tile and its apron; pixels beyond the image (ragged tiles) read as 0 and only feed windows that are not counted
  for (int i = t; i < SS_IH * SS_IW; i += EM_THREADS) {
    const int r = i / SS_IW, c = i % SS_IW, y = y0 + r, x = x0 + c;
    const bool in = y < H && x < W;
    const int64_t at = (int64_t)y * W + x;
    sp[r][c] = in ? clamp_keep_nan(pred[at], lo, hi) : 0.0f;
    sg[r][c] = in ? clamp_keep_nan(gt[at], lo, hi) : 0.0f;
  }
  __syncthreads();
  mn = waves_combine<EM_WAVES>(sh_min, RedMin());
  mx = waves_combine<EM_WAVES>(sh_max, RedMax());
  const double R = (double)mx - (double)mn;
  const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);
  for (int i = t; i < SS_IH * SS_TW; i += EM_THREADS) {
    const int r = i / SS_TW, c = i % SS_TW;
    double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {
      const double p = (double)sp[r][c + k], g = (double)sg[r][c + k];
      a += p;
      b += g;
      aa += p * p;
      bb += g * g;
      ab += p * g;
    }
    rows[0][r][c] = a;
    rows[1][r][c] = b;
    rows[2][r][c] = aa;
    rows[3][r][c] = bb;
    rows[4][r][c] = ab;
  }
  __syncthreads();
  // window means by a true division, as the formula has it: where the sums of a constant image are exact (49 c^2 representable),
  // uxx - ux*ux is exactly 0 as it is in numpy; otherwise the R = 0 case is rounding noise over rounding noise on both sides
  const double n_px = (double)(SS_WIN * SS_WIN), cov_norm = n_px / (n_px - 1.0);
  double acc = 0.0;
  for (int i = t; i < SS_TH * SS_TW; i += EM_THREADS) {
    const int r = i / SS_TW, c = i % SS_TW;
    if (y0 + r > H - SS_WIN || x0 + c > W - SS_WIN) continue;
    double s[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < SS_WIN; ++k) v += rows[q][r + k][c];
      s[q] = v / n_px;
    }
    const double ux = s[0], uy = s[1];
    const double vx = cov_norm * (s[2] - ux * ux), vy = cov_norm * (s[3] - uy * uy), vxy = cov_norm * (s[4] - ux * uy);
    acc += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
  }
  acc = block_reduce<EM_WAVES>(acc, sh_sum, RedSum());
  if (t == 0) part_ssim[blockIdx.x] = acc;
}

// ---- results --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EM_THREADS) eval_finalize_kernel(const uint32_t* __restrict__ hist, const double* __restrict__ part_sq,
                                                                  int n_part, const double* __restrict__ part_ssim, int n_tiles, int n,
                                                                  int H, int W, float hi, double* __restrict__ out) {
  __shared__ double sh_sum[EM_WAVES];
  __shared__ uint32_t sh_key[2];
  const int t = threadIdx.x;
  double sq = 0.0, ss = 0.0;
  for (int i = t; i < n_part; i += EM_THREADS) sq += part_sq[i];
  for (int i = t; i < n_tiles; i += EM_THREADS) ss += part_ssim[i];
  sq = block_reduce<EM_WAVES>(sq, sh_sum, RedSum());
  ss = block_reduce<EM_WAVES>(ss, sh_sum, RedSum());
  if (t < 64) {
    uint32_t k0 = (uint32_t)(n - 1) >> 1, k1 = (uint32_t)n >> 1;
    const uint32_t a = select_prefix(hist, EM_PASSES, 0, k0), b = select_prefix(hist, EM_PASSES, 1, k1);
    if (t == 0) { sh_key[0] = a; sh_key[1] = b; }
  }
  __syncthreads();
  if (t != 0) return;
  const double mse = sq / (double)n;
  const float a = __uint_as_float(sh_key[0]), b = __uint_as_float(sh_key[1]);
  // numpy's median: the middle value, or the fp32 mean of the two middle values; NaN as soon as one |d| is (then sq is)
  const float med = (n & 1) ? a : (a + b) / 2.0f;
  out[0] = sqrt(mse);
  out[1] = sq != sq ? (double)__builtin_nanf("") : (double)med;
  out[2] = ss / ((double)(H - (SS_WIN - 1)) * (double)(W - (SS_WIN - 1)));
  out[3] = 10.0 * log10((double)hi * (double)hi / mse);
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
extern "C" int64_t l4de_image_errors_workspace(int32_t H, int32_t W) {
  return eval_shape_ok(H, W) ? eval_ws_carve(nullptr, H, W, nullptr) : 0;
}

extern "C" int l4de_image_errors(const float* pred, const float* gt, int32_t H, int32_t W, float lo, float hi, double* out,
                                 void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (H < SS_WIN || W < SS_WIN) L4D_FAIL("l4de_image_errors: H and W must be at least 7 (one SSIM window)");
  if (!eval_shape_ok(H, W)) L4D_FAIL("l4de_image_errors: more than 2^28 pixels");
  if (!pred || !gt || !out || !workspace) L4D_FAIL("l4de_image_errors: null pointer");
  if (((uintptr_t)workspace & 7) != 0) L4D_FAIL("l4de_image_errors: workspace must be 8-byte aligned");
  EvalWs ws;
  eval_ws_carve(workspace, H, W, &ws);
  const int n = H * W;
  const int64_t chunks = ceil_div64(n, EM_CHUNK);
  const int blocks = (int)(chunks < EM_MAX_BLOCKS ? chunks : EM_MAX_BLOCKS);
  const int tiles_x = (int)ceil_div64(W - (SS_WIN - 1), SS_TW), tiles = (int)ssim_tiles(H, W);
  l4d_fill_async(ws.hist, 0u, EM_PASSES * 2 * 256 * 4, stream);
  L4D_LAUNCH(eval_errors_kernel, dim3(blocks), dim3(EM_THREADS), 0, stream, pred, gt, n, lo, hi, ws.absd, ws.hist, ws.part_sq,
             ws.part_min, ws.part_max);
  L4D_LAUNCH(eval_ssim_kernel, dim3(tiles), dim3(EM_THREADS), 0, stream, pred, gt, (int)H, (int)W, lo, hi, (const float*)ws.part_min,
             (const float*)ws.part_max, blocks, tiles_x, ws.part_ssim);
  for (int pass = 1; pass < EM_PASSES; ++pass)
    L4D_LAUNCH(eval_select_kernel, dim3(blocks), dim3(EM_THREADS), 0, stream, (const uint32_t*)ws.absd, n, pass, ws.hist);
  L4D_LAUNCH(eval_finalize_kernel, dim3(1), dim3(EM_THREADS), 0, stream, (const uint32_t*)ws.hist, (const double*)ws.part_sq, blocks,
             (const double*)ws.part_ssim, tiles, n, (int)H, (int)W, hi, out);
  L4D_LAUNCH_CHECK("l4de_image_errors");
  return 0;
}
