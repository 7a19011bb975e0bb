// The fused bias-free ReLU MLP of mlp.hip for the hidden widths 16, 32 and 128 (tiny-cuda-nn's FullyFusedMLP accepts 16, 32, 64 and
// 128 neurons; main_lidar4d.py:53-59 --hidden_dim_sigma / --hidden_dim_lidar / --hidden_dim_flow): liblidar4d_mlp.so,
// include/lidar4d_mlp.h.  Width 64 stays in mlp.hip, tuned for the default model; this file is ONE template on the width, with the
// input width and (forward) the depth as run-time values, and is not tuned.
//
// Operand layouts, the permuted weight-row order that makes a layer's C fragment the next layer's B fragment, and the wave-private
// LDS image that turns the chain layout into the batch-major operands of dW = dZ^T H (ds_write_b128, ds_read_b64_tr_b16): mlp.hip's
// header comment and mlp_dev.h, whose pieces are used as they are.  What differs:
//   * HP = max(width, 32) neurons are computed: a K step of v_mfma_f32_16x16x32_f16 is 32 wide, so width 16 runs as width 32 whose
//     upper 16 neurons have zero weights (never stored: act and grad_w have `width` columns).  HT = HP / 16 neuron tiles, KS = HP / 32
//     K steps.
//   * Every weight fragment of the network lives in LDS (dynamic: up to 116 KB forward, 148 KB backward at width 128).
//   * Backward, width 128: a hidden layer's dW is 16,384 fp32 values -- 256 registers per lane if one wavefront held it.  The four
//     wavefronts of a workgroup therefore take the SAME 32-row tile, each runs the whole dZ chain (its own staging image, no barrier)
//     and each accumulates the dW rows of its own quarter of the neuron tiles (SPLIT).  dX is a launch of its own there: its W1^T
//     fragments do not fit LDS next to the staging images.  Widths 16 and 32: one launch, a wavefront per tile, as in mlp.hip.
//   * The ReLU gate is the comparison act > 0 (mlp.hip's integer form needs an activation that is never -0).
// Rows at or past the row count are neither read nor written: their operands are staged as the zeros they are, so the MFMAs and
// the transposing reads run in wave-uniform control flow with EXEC all ones.
#include "common.h"
#include "wave_dev.h"

#include "mlp_dev.h"

#include "../../include/lidar4d_mlp.h"

extern "C" int l4dm_version(void) { return L4DM_ABI_VERSION; }
extern "C" const char* l4dm_last_error(void) { return l4d_last_error(); }

#define MLPW_MAX_IN_TILES 12  // in_pad <= 192

template <int W>
struct Width {
  static constexpr int HP = W < 32 ? 32 : W;  // neurons computed
  static constexpr int HT = HP / 16;          // 16-neuron tiles
  static constexpr int KS = HP / 32;          // 32-wide K steps over a hidden vector
};

__device__ __forceinline__ h8 as_h8(const uint4& u) { return *reinterpret_cast<const h8*>(&u); }

// ================================================================================================
// forward
// ================================================================================================
// fragments: layer 1 [HT][ks_in], hidden layers 2 .. nh [HT][KS] each, output [KS]
template <int W>
__global__ void __launch_bounds__(256) mlpw_fwd_kernel(const half_t* __restrict__ x, int64_t cap, const int32_t* __restrict__ n_rows,
                                                      int in_pad, int nh, const half_t* __restrict__ weights,
                                                      half_t* __restrict__ y, half_t* __restrict__ act, float* __restrict__ sigma) {
  constexpr int HT = Width<W>::HT, KS = Width<W>::KS;
  const int64_t P = n_rows ? min((int64_t)*n_rows, cap) : cap;
  const int ks_in = (in_pad + 31) / 32;
  const int nf_l1 = HT * ks_in, nf_h = HT * KS;
  const int nf = nf_l1 + (nh - 1) * nf_h + KS;
  extern __shared__ uint4 lds[];  // [nf][64]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  for (int f = wave; f < nf; f += 4) {
    h8 v;
    if (f < nf_l1) {
      const int mt = f / ks_in, ks = f % ks_in;
      v = build_frag(weights, W, in_pad, 0, perm_row(mt, i), 32 * ks + 8 * g);
    } else if (f < nf - KS) {
      const int q = f - nf_l1, layer = q / nf_h, mt = (q % nf_h) / KS, ks = q % KS;
      v = build_frag(weights + W * in_pad + layer * W * W, W, W, 0, perm_row(mt, i), 32 * ks + 8 * g);
    } else {
      const int ks = f - (nf - KS);
      v = build_frag(weights + W * in_pad + (nh - 1) * W * W, 16, W, 0, i, 32 * ks + 8 * g);
    }
    lds[f * 64 + lane] = *reinterpret_cast<uint4*>(&v);
  }
  __syncthreads();
  auto FR = [&](int f) -> h8 { return as_h8(lds[f * 64 + lane]); };

  const int64_t n_tiles = (P + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row = tile * 16 + i;
    const bool ok = row < P;
    f4 acc[HT];
#pragma unroll
    for (int mt = 0; mt < HT; ++mt) acc[mt] = f4{0, 0, 0, 0};
    for (int ks = 0; ks < ks_in; ++ks) {
      const int k0 = 32 * ks + 8 * g;
      uint4 u = make_uint4(0, 0, 0, 0);
      if (ok && k0 < in_pad) u = *reinterpret_cast<const uint4*>(x + row * in_pad + k0);
      const h8 xb = as_h8(u);
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) acc[mt] = MFMA(FR(mt * ks_in + ks), xb, acc[mt]);
    }
    h8 hb[KS];
    for (int l = 0;; ++l) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        hb[ks] = relu_pack(acc[2 * ks], acc[2 * ks + 1]);
        if (act && ok && 32 * ks + 8 * g < W) *reinterpret_cast<h8*>(act + ((int64_t)l * cap + row) * W + 32 * ks + 8 * g) = hb[ks];
      }
      if (l + 1 >= nh) break;
      const int base = nf_l1 + l * nf_h;
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) {
        acc[mt] = f4{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc[mt] = MFMA(FR(base + mt * KS + ks), hb[ks], acc[mt]);
      }
    }
    // output layer: C[m = 4g + r][row i]
    f4 o = f4{0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) o = MFMA(FR(nf - KS + ks), hb[ks], o);
    if (ok) {
      h4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = f2h(clamp_h(o[r]));
      *reinterpret_cast<h4*>(y + row * 16 + 4 * g) = ov;
      if (sigma && g == 0) sigma[row] = expf(h2f(ov[0]));
    }
  }
}

// ================================================================================================
// backward
// ================================================================================================
// DxStat: *out = max(*out, max |dx[:, 16 lo_tile : 16 hi_tile]|) over the rows of the launch, as stored (+inf for a non-finite value)
struct DxStat {
  float* out;
  int lo_tile, hi_tile;
};

// fragments: Wo^T [HT] (one K step: 16 outputs, zero-filled to 32), hidden W_l^T for l = NH .. 2 [HT][KS] each, then (DO_DX) W1^T
// in natural row order [in_tiles][KS].  Behind them (DO_DW) two staging images per wavefront: one reused for dy, every layer's
// activations and x in 32-column chunks, one for dZ.
// DO_DW: accumulate the weight gradients; DO_DX: produce dx.  SPLIT (DO_DW at width 128): see the header comment.
template <int W, int NH, bool DO_DW, bool DO_DX>
__global__ void __launch_bounds__(256) mlpw_bwd_kernel(const half_t* __restrict__ x, const half_t* __restrict__ act,
                                                      const half_t* __restrict__ dy, int64_t cap, const int32_t* __restrict__ n_rows,
                                                      int in_pad, const half_t* __restrict__ weights, half_t* __restrict__ dx,
                                                      float* __restrict__ grad_w, float inv_scale, DxStat dstat) {
  constexpr int HT = Width<W>::HT, KS = Width<W>::KS;
  constexpr bool SPLIT = DO_DW && W == 128;
  constexpr int OWN = SPLIT ? HT / 4 : HT;  // neuron tiles whose dW rows (output layer: dW columns) this wavefront accumulates
  const int64_t P = n_rows ? min((int64_t)*n_rows, cap) : cap;
  const int in_tiles = in_pad / 16, ks_in = (in_tiles + 1) / 2;
  constexpr int WOT = 0, WH = HT, W1T = WH + (NH - 1) * HT * KS;
  const int nf = W1T + (DO_DX ? in_tiles * KS : 0);
  using SG = BwdStage<KS>;
  extern __shared__ uint4 lds[];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int mt0 = SPLIT ? wave * OWN : 0;
  lds_u8* const stage_base = reinterpret_cast<lds_u8*>((__attribute__((address_space(3))) void*)&lds[nf * 64 + wave * (2 * SG::BYTES / 16)]);
  lds_u8* const stage_wr = stage_base + (i >> 2) * SG::BLK + (i & 3) * SG::PITCH + 16 * g;
  lds_u8* const stage_rd = stage_base + g * SG::BLK + (i >> 2) * SG::PITCH + 8 * (i & 3);
  const half_t* Wo = weights + W * in_pad + (NH - 1) * W * W;

  for (int f = wave; f < nf; f += 4) {
    h8 v;
    if (f < WH) {
      v = build_frag(Wo, 16, W, 1, perm_row(f, i), 8 * g);  // k = output index (only 16 real)
    } else if (f < W1T) {
      const int q = f - WH, li = q / (HT * KS), r = q % (HT * KS);  // li = 0 -> layer NH, 1 -> NH - 1 ...
      const half_t* Wl = weights + W * in_pad + (NH - li - 2) * W * W;
      v = build_frag(Wl, W, W, 1, perm_row(r / KS, i), 32 * (r % KS) + 8 * g);
    } else {
      const int q = f - W1T;
      v = build_frag(weights, W, in_pad, 1, 16 * (q / KS) + i, 32 * (q % KS) + 8 * g);
    }
    lds[f * 64 + lane] = *reinterpret_cast<uint4*>(&v);
  }
  __syncthreads();
  auto FR = [&](int f) -> h8 { return as_h8(lds[f * 64 + lane]); };

  // dW accumulators, C layout: [m = 16 mt + 4g + r][k = 16 nt + i]
  f4 dWo[OWN];                                 // [16 outputs][neuron tile mt0 + q]
  f4 dWh[NH > 1 ? NH - 1 : 1][OWN][HT];        // [neuron tile mt0 + q][input neuron tile]
  f4 dW1[OWN][MLPW_MAX_IN_TILES];              // [neuron tile mt0 + q][input column tile]; tiles >= in_tiles stay untouched
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    dWo[q] = f4{0, 0, 0, 0};
#pragma unroll
    for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l)
#pragma unroll
      for (int nt = 0; nt < HT; ++nt) dWh[l][q][nt] = f4{0, 0, 0, 0};
#pragma unroll
    for (int nt = 0; nt < MLPW_MAX_IN_TILES; ++nt) dW1[q][nt] = f4{0, 0, 0, 0};
  }
  float dx_amax = 0.0f;

  const int64_t n_macro = (P + 31) / 32;
  const int64_t tile_stride = SPLIT ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  for (int64_t mtile = SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave; mtile < n_macro; mtile += tile_stride) {
    asm volatile("" ::: "memory");
    int64_t rows[2];
    bool ok[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      rows[a] = mtile * 32 + 8 * (i >> 2) + 4 * a + (i & 3);
      ok[a] = rows[a] < P;
    }
    // x of the tile, chain layout, requested here so that its loads fly under the whole dZ chain -- where the registers allow it:
    // not next to SPLIT's accumulators of three hidden layers (490 of 512 registers without it).  Measured at 12.6 M rows, width 128,
    // in_pad 128, one hidden layer: 8.58 -> 5.22 ms (one wavefront per SIMD there: nothing else hides the loads)
    constexpr bool PRELOAD_X = DO_DW && (!SPLIT || NH <= 2);
    uint4 xv[2][PRELOAD_X ? MLPW_MAX_IN_TILES / 2 : 1];
    auto load_x = [&](int a, int ks) -> uint4 {
      uint4 u = make_uint4(0, 0, 0, 0);
      if (ok[a] && 32 * ks + 8 * g < in_pad) u = *reinterpret_cast<const uint4*>(x + rows[a] * in_pad + 32 * ks + 8 * g);
      return u;
    };
    if (PRELOAD_X) {
#pragma unroll
      for (int ks = 0; ks < MLPW_MAX_IN_TILES / 2; ++ks)
        if (ks < ks_in) {  // wave-uniform
#pragma unroll
          for (int a = 0; a < 2; ++a) xv[a][PRELOAD_X ? ks : 0] = load_x(a, ks);
        }
    }
    // activations of hidden layer `layer` (1-based), chain layout [a][ks]; columns past the width and rows past the end are zeros
    auto load_hidden = [&](int layer, uint4 (&h)[2][KS]) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          h[a][ks] = make_uint4(0, 0, 0, 0);
          if (ok[a] && 32 * ks + 8 * g < W)
            h[a][ks] = *reinterpret_cast<const uint4*>(act + ((int64_t)(layer - 1) * cap + rows[a]) * W + 32 * ks + 8 * g);
        }
    };
    // chain layout -> batch-major (rows 8g .. 8g + 7 of feature 16 nt + i) through the first image.  The transposed reads are
    // issued behind the section's chain MFMAs, right in front of the dW MFMAs that consume them: held across the chain they cost
    // the width-128 kernels the registers that their accumulators need.
    auto stage_hidden = [&](const uint4 (&h)[2][KS]) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) stage_write<SG::PITCH>(stage_wr, a, ks, h[a][ks]);
      asm volatile("" ::: "memory");
    };
    // the gated dZ of a layer -> batch-major, the tiles this wavefront owns, through the second image
    auto stage_dz = [&](const h8 (&nz)[2][KS], h8 (&zT)[OWN]) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) stage_write<SG::PITCH>(stage_wr + SG::BYTES, a, ks, *reinterpret_cast<const uint4*>(&nz[a][ks]));
#pragma unroll
      for (int q = 0; q < OWN; ++q) zT[q] = stage_read_t<SG::PITCH>(stage_rd + SG::BYTES, mt0 + q);
      asm volatile("" ::: "memory");
    };
    // ReLU': c (fp32, chain tiles 2 ks and 2 ks + 1) rounded to fp16 where the activation is > 0, else 0
    auto gate = [&](const f4 (&c)[HT], const uint4 (&h)[KS], h8 (&nz)[KS]) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const h8 hv = as_h8(h[ks]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          nz[ks][r] = hv[r] > (half_t)0.0f ? f2h_grad(c[2 * ks][r]) : (half_t)0.0f;
          nz[ks][4 + r] = hv[4 + r] > (half_t)0.0f ? f2h_grad(c[2 * ks + 1][r]) : (half_t)0.0f;
        }
      }
    };

    // ---- output layer --------------------------------------------------------------------------
    uint4 dyv[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      dyv[a] = make_uint4(0, 0, 0, 0);  // k = 16 .. 31 of the output contraction do not exist
      if (ok[a] && g < 2) dyv[a] = *reinterpret_cast<const uint4*>(dy + rows[a] * 16 + 8 * g);
    }
    uint4 hc[2][KS];
    load_hidden(NH, hc);
    h8 dyT, dzT[OWN];
    if (DO_DW) {
#pragma unroll
      for (int a = 0; a < 2; ++a) stage_write<SG::PITCH>(stage_wr, a, 0, dyv[a]);
      dyT = stage_read_t<SG::PITCH>(stage_rd, 0);
      stage_hidden(hc);
    }
    h8 dzf[2][KS];  // chain B fragments of the current layer's dZ
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f4 c[HT];
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) c[mt] = MFMA(FR(WOT + mt), as_h8(dyv[a]), (f4{0, 0, 0, 0}));
      gate(c, hc[a], dzf[a]);
    }
    if (DO_DW) {
#pragma unroll
      for (int q = 0; q < OWN; ++q) dWo[q] = MFMA(dyT, stage_read_t<SG::PITCH>(stage_rd, mt0 + q), dWo[q]);
      stage_dz(dzf, dzT);
    }
    // ---- hidden layers NH .. 2 -----------------------------------------------------------------
#pragma unroll
    for (int li = 0; li < NH - 1; ++li) {
      const int layer = NH - li;  // the current dZ belongs to hidden layer `layer`; its input is H_{layer - 1}
      load_hidden(layer - 1, hc);
      if (DO_DW) stage_hidden(hc);
      h8 nz[2][KS];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        f4 c[HT];
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {
          c[mt] = f4{0, 0, 0, 0};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) c[mt] = MFMA(FR(WH + (li * HT + mt) * KS + ks), dzf[a][ks], c[mt]);
        }
        gate(c, hc[a], nz[a]);
      }
      if (DO_DW) {
#pragma unroll
        for (int nt = 0; nt < HT; ++nt) {
          const h8 hT = stage_read_t<SG::PITCH>(stage_rd, nt);
#pragma unroll
          for (int q = 0; q < OWN; ++q) dWh[layer - 2][q][nt] = MFMA(dzT[q], hT, dWh[layer - 2][q][nt]);
        }
        asm volatile("" ::: "memory");
        stage_dz(nz, dzT);  // (dzT's last use is just above)
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) dzf[a][ks] = nz[a][ks];
    }
    // ---- first layer: dW1 = dZ1^T X, dX = dZ1 W1 -----------------------------------------------
    if (DO_DW) {
      asm volatile("" ::: "memory");  // (the chunks of x go where the last activations were: behind their reads)
#pragma unroll
      for (int ks = 0; ks < MLPW_MAX_IN_TILES / 2; ++ks) {
        if (ks < ks_in) {  // wave-uniform
#pragma unroll
          for (int a = 0; a < 2; ++a) stage_write<SG::PITCH>(stage_wr, a, 0, PRELOAD_X ? xv[a][PRELOAD_X ? ks : 0] : load_x(a, ks));
          const h8 xT0 = stage_read_t<SG::PITCH>(stage_rd, 0);
          const h8 xT1 = stage_read_t<SG::PITCH>(stage_rd, 1);  // (an odd tile count: zeros, and an accumulator that is never flushed)
          asm volatile("" ::: "memory");
#pragma unroll
          for (int q = 0; q < OWN; ++q) {
            dW1[q][2 * ks] = MFMA(dzT[q], xT0, dW1[q][2 * ks]);
            dW1[q][2 * ks + 1] = MFMA(dzT[q], xT1, dW1[q][2 * ks + 1]);
          }
        }
      }
    }
    if (DO_DX && dx) {
      for (int mt = 0; mt < in_tiles; ++mt) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          f4 c = f4{0, 0, 0, 0};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) c = MFMA(FR(W1T + mt * KS + ks), dzf[a][ks], c);
          if (ok[a]) {
            h4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = f2h_grad(c[r]);
            *reinterpret_cast<h4*>(dx + rows[a] * in_pad + 16 * mt + 4 * g) = ov;
            if (dstat.out && mt >= dstat.lo_tile && mt < dstat.hi_tile) {
#pragma unroll
              for (int r = 0; r < 4; ++r) dx_amax = amax_nf(dx_amax, h2f(ov[r]));
            }
          }
        }
      }
    }
  }

  if (DO_DX && dstat.out) {  // wave-uniform
    dx_amax = wave_max(dx_amax);
    if (lane == 0 && dx_amax > 0.0f) atomic_max_nonneg(dstat.out, dx_amax);
  }
  if (!DO_DW) return;
  // ---- flush dW (fp32 atomics; one add per element per wavefront); rows / columns of the zero-filled neurons do not exist ------
  float* gWo = grad_w + W * in_pad + (NH - 1) * W * W;
#pragma unroll
  for (int q = 0; q < OWN; ++q)
#pragma unroll
    for (int nt = 0; nt < MLPW_MAX_IN_TILES; ++nt)
      if (nt < in_tiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = 16 * (mt0 + q) + 4 * g + r;
          const float v = dW1[q][nt][r] * inv_scale;
          if (m < W && v != 0.0f) atomicAdd(grad_w + m * in_pad + 16 * nt + i, v);
        }
      }
#pragma unroll
  for (int l = 0; l < NH - 1; ++l) {
    float* gWl = grad_w + W * in_pad + l * W * W;
#pragma unroll
    for (int q = 0; q < OWN; ++q)
#pragma unroll
      for (int nt = 0; nt < HT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = 16 * (mt0 + q) + 4 * g + r, n = 16 * nt + i;
          const float v = dWh[l][q][nt][r] * inv_scale;
          if (m < W && n < W && v != 0.0f) atomicAdd(gWl + m * W + n, v);
        }
  }
#pragma unroll
  for (int q = 0; q < OWN; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 16 * (mt0 + q) + i;
      const float v = dWo[q][r] * inv_scale;
      if (n < W && v != 0.0f) atomicAdd(gWo + (4 * g + r) * W + n, v);
    }
}

// ================================================================================================
// C ABI
// ================================================================================================
// Workgroups per launch (wavefronts grid-stride over the rest).  Every workgroup builds the network's fragments first, and every
// wavefront of a backward launch ends with a flush of its dW, so no more workgroups than keep the chip busy.  Rows per pass:
//   forward  width 16 / 32: 1024 x 4 x 16 = 65,536    width 128: 256 x 4 x 16 = 16,384  (one workgroup per CU: its LDS)
//   backward width 16 / 32:  512 x 4 x 32 = 65,536    width 128: dW 256 x 32 = 8,192, dX 256 x 4 x 32 = 32,768
#define MLPW_FWD_GRID_NARROW 1024
#define MLPW_BWD_GRID_NARROW 512
#define MLPW_GRID_WIDE 256

static int grid_for(int64_t jobs, int cap) { return (int)(jobs < 1 ? 1 : (jobs > cap ? cap : jobs)); }

// LDS beyond 64 KB has to be asked for, once per kernel
template <typename K>
static bool allow_lds(K kernel, size_t bytes) {
  return bytes <= 65536 || hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

static bool shape_ok(int32_t in_pad, int32_t hidden, int32_t n_hidden) {
  const bool w = hidden == 16 || hidden == 32 || hidden == 128;
  const bool in = in_pad == 16 || in_pad == 32 || in_pad == 64 || in_pad == 96 || in_pad == 128 || in_pad == 160 || in_pad == 176 || in_pad == 192;
  return w && in && n_hidden >= 1 && n_hidden <= 3;
}

template <int W>
static int fwd_launch(const void* x, int64_t cap, const int32_t* n_rows, int32_t in_pad, int32_t n_hidden, const void* weights, void* y,
                      void* act, float* sigma, void* stream) {
  constexpr int HT = Width<W>::HT, KS = Width<W>::KS;
  const int nf = HT * ((in_pad + 31) / 32) + (n_hidden - 1) * HT * KS + KS;
  const size_t lds = (size_t)nf * 1024;
  if (!allow_lds(mlpw_fwd_kernel<W>, lds)) L4D_FAIL("l4dm_mlp_fwd: the device refuses the kernel's LDS size");
  const int grid = grid_for((cap + 63) / 64, W == 128 ? MLPW_GRID_WIDE : MLPW_FWD_GRID_NARROW);
  L4D_LAUNCH((mlpw_fwd_kernel<W>), dim3(grid), dim3(256), lds, (hipStream_t)stream, (const half_t*)x, cap, n_rows, (int)in_pad,
             (int)n_hidden, (const half_t*)weights, (half_t*)y, (half_t*)act, sigma);
  return 0;
}

extern "C" int l4dm_mlp_fwd(const void* x, int64_t cap, const int32_t* n_rows, int32_t in_pad, int32_t hidden, int32_t n_hidden,
                            const void* weights, void* y, void* act, float* sigma, void* stream) {
  if (!shape_ok(in_pad, hidden, n_hidden))
    L4D_FAIL("l4dm_mlp_fwd: unsupported shape; hidden in {16,32,128} (64: l4d_mlp_fwd), in_pad in {16,32,64,96,128,160,176,192}, n_hidden in 1..3");
  if (cap < 0 || !x || !weights || !y) L4D_FAIL("l4dm_mlp_fwd: x, weights and y are required, cap >= 0");
  if (cap == 0) return 0;
  int rc = 0;
  if (hidden == 16) rc = fwd_launch<16>(x, cap, n_rows, in_pad, n_hidden, weights, y, act, sigma, stream);
  else if (hidden == 32) rc = fwd_launch<32>(x, cap, n_rows, in_pad, n_hidden, weights, y, act, sigma, stream);
  else rc = fwd_launch<128>(x, cap, n_rows, in_pad, n_hidden, weights, y, act, sigma, stream);
  if (rc) return rc;
  L4D_LAUNCH_CHECK("l4dm_mlp_fwd");
  return 0;
}

template <int W, int NH>
static int bwd_launch(const void* x, const void* act, const void* dy, int64_t cap, const int32_t* n_rows, int32_t in_pad,
                      const void* weights, void* dx, float* grad_w, float inv_scale, DxStat dstat, void* stream) {
  constexpr int HT = Width<W>::HT, KS = Width<W>::KS;
  constexpr size_t STAGE = 4 * 2 * (size_t)BwdStage<KS>::BYTES;  // four wavefronts, two images each
  const int nf_chain = HT + (NH - 1) * HT * KS, nf_dx = (in_pad / 16) * KS;
  const int64_t n_macro = (cap + 31) / 32;
#define MLPW_BWD(DW, DX, lds_bytes, grid)                                                                                      \
  do {                                                                                                                         \
    if (!allow_lds(mlpw_bwd_kernel<W, NH, DW, DX>, lds_bytes)) L4D_FAIL("l4dm_mlp_bwd: the device refuses the kernel's LDS size"); \
    L4D_LAUNCH((mlpw_bwd_kernel<W, NH, DW, DX>), dim3(grid), dim3(256), lds_bytes, (hipStream_t)stream, (const half_t*)x,      \
               (const half_t*)act, (const half_t*)dy, cap, n_rows, (int)in_pad, (const half_t*)weights, (half_t*)dx, grad_w,   \
               inv_scale, dstat);                                                                                              \
  } while (0)
  if constexpr (W == 128) {
    MLPW_BWD(true, false, (size_t)nf_chain * 1024 + STAGE, grid_for(n_macro, MLPW_GRID_WIDE));
    if (dx) MLPW_BWD(false, true, (size_t)(nf_chain + nf_dx) * 1024, grid_for((n_macro + 3) / 4, MLPW_GRID_WIDE));
  } else {
    MLPW_BWD(true, true, (size_t)(nf_chain + nf_dx) * 1024 + STAGE, grid_for((n_macro + 3) / 4, MLPW_BWD_GRID_NARROW));
  }
#undef MLPW_BWD
  return 0;
}

extern "C" int l4dm_mlp_bwd(const void* x, const void* act, const void* dy, int64_t cap, const int32_t* n_rows, int32_t in_pad,
                            int32_t hidden, int32_t n_hidden, const void* weights, void* dx, float* grad_w, float inv_scale,
                            float* dx_absmax, int32_t absmax_lo, int32_t absmax_hi, void* stream) {
  if (!shape_ok(in_pad, hidden, n_hidden))
    L4D_FAIL("l4dm_mlp_bwd: unsupported shape; hidden in {16,32,128} (64: l4d_mlp_bwd), in_pad in {16,32,64,96,128,160,176,192}, n_hidden in 1..3");
  if (cap < 0 || !x || !act || !dy || !weights || !grad_w)
    L4D_FAIL("l4dm_mlp_bwd: x, act (the activations are not recomputed), dy, weights and grad_w are required, cap >= 0");
  if (dx_absmax && (absmax_lo % 16 || absmax_hi % 16 || absmax_lo < 0 || absmax_hi > in_pad || !dx))
    L4D_FAIL("l4dm_mlp_bwd: dx_absmax needs dx and a column range in multiples of 16 inside [0, in_pad]");
  if (cap == 0) return 0;
  const DxStat dstat{dx_absmax, absmax_lo / 16, absmax_hi / 16};
  int rc = 0;
#define X(WW, NHH)                               \
  if (hidden == WW && n_hidden == NHH)           \
    rc = bwd_launch<WW, NHH>(x, act, dy, cap, n_rows, in_pad, weights, dx, grad_w, inv_scale, dstat, stream);
  X(16, 1) X(16, 2) X(16, 3) X(32, 1) X(32, 2) X(32, 3) X(128, 1) X(128, 2) X(128, 3)
#undef X
  if (rc) return rc;
  L4D_LAUNCH_CHECK("l4dm_mlp_bwd");
  return 0;
}
