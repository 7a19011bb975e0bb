// The un-fused hex-plane sampler, forward and backward, on the channel count C: the kernels planes.hip (C = 8, liblidar4d_hip.so)
// and planes_width.hip (C = 4, 8, 16, liblidar4d_planes.so) both launch, and the descriptor check in front of them.  One thread per
// sample, plane gradients through global fp32 atomics.
#pragma once
#include "planes_dev.h"

template <int C>
__global__ void __launch_bounds__(256) planes_fwd_kernel(PlaneDesc desc, const float* __restrict__ arena,
                                                        const float* __restrict__ xt, int64_t P, int which,
                                                        float* __restrict__ out_s, float* __restrict__ out_d) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float4_t c4 = *reinterpret_cast<const float4_t*>(xt + p * 4);
  const float coord[4] = {c4[0], c4[1], c4[2], c4[3]};
  const int n_out = desc.n_scales * C;
  for (int s = 0; s < desc.n_scales; ++s) {
    float fs[C], fd[C];
    bool first_s = true, first_d = true;
#pragma unroll
    for (int ci = 0; ci < NPLANES; ++ci) {
      const int a = COMB_A[ci], b = COMB_B[ci];
      const bool is_t = (b == 3);
      if ((which == 1 && is_t) || (which == 2 && !is_t)) continue;
      Tap t;
      const int W = desc.res[s][a], H = desc.res[s][b];
      axis_tap(coord[a], W, t.x0, t.x1, t.wx0, t.wx1, t.mx);
      axis_tap(coord[b], H, t.y0, t.y1, t.wy0, t.wy1, t.my);
      float v[C];
      sample_plane<C>(arena + desc.off[s][ci], W, t, v);
      if (is_t) {
#pragma unroll
        for (int k = 0; k < C; ++k) fd[k] = first_d ? v[k] : fd[k] * v[k];
        first_d = false;
      } else {
#pragma unroll
        for (int k = 0; k < C; ++k) fs[k] = first_s ? v[k] : fs[k] * v[k];
        first_s = false;
      }
    }
    if (which != 2) {
      float4_t* o = reinterpret_cast<float4_t*>(out_s + p * n_out + s * C);
#pragma unroll
      for (int q = 0; q < C / 4; ++q) o[q] = float4_t{fs[q * 4], fs[q * 4 + 1], fs[q * 4 + 2], fs[q * 4 + 3]};
    }
    if (which != 1) {
      float4_t* o = reinterpret_cast<float4_t*>(out_d + p * n_out + s * C);
#pragma unroll
      for (int q = 0; q < C / 4; ++q) o[q] = float4_t{fd[q * 4], fd[q * 4 + 1], fd[q * 4 + 2], fd[q * 4 + 3]};
    }
  }
}

// One group of three planes (static: xy, xz, yz; time: xt, yt, zt) of scale s at `coord`: taps, interpolated values, and -- given the
// gradient g of the group's product -- the scatter into the planes' gradients and the gradient towards the four coordinates.
template <int C>
struct Group {
  Tap taps[3];
  float v[3][C];
};
__device__ __forceinline__ int group_plane(bool time_group, int j) { return time_group ? (j == 0 ? 2 : j == 1 ? 4 : 5) : (j == 0 ? 0 : j == 1 ? 1 : 3); }

template <int C>
__device__ __forceinline__ void group_sample(const PlaneDesc& desc, const float* __restrict__ arena, int s, bool time_group,
                                             const float coord[4], Group<C>& g, float prod[C]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int ci = group_plane(time_group, j);
    const int a = COMB_A[ci], b = COMB_B[ci];
    const int W = desc.res[s][a], H = desc.res[s][b];
    axis_tap(coord[a], W, g.taps[j].x0, g.taps[j].x1, g.taps[j].wx0, g.taps[j].wx1, g.taps[j].mx);
    axis_tap(coord[b], H, g.taps[j].y0, g.taps[j].y1, g.taps[j].wy0, g.taps[j].wy1, g.taps[j].my);
    sample_plane<C>(arena + desc.off[s][ci], W, g.taps[j], g.v[j]);
#pragma unroll
    for (int k = 0; k < C; ++k) prod[k] = j == 0 ? g.v[j][k] : prod[k] * g.v[j][k];
  }
}

// the product alone (forward): nothing of the taps is kept
template <int C>
__device__ __forceinline__ void group_product(const PlaneDesc& desc, const float* __restrict__ arena, int s, bool time_group,
                                              const float coord[4], float prod[C]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int ci = group_plane(time_group, j);
    const int a = COMB_A[ci], b = COMB_B[ci];
    const int W = desc.res[s][a], H = desc.res[s][b];
    Tap t;
    axis_tap(coord[a], W, t.x0, t.x1, t.wx0, t.wx1, t.mx);
    axis_tap(coord[b], H, t.y0, t.y1, t.wy0, t.wy1, t.my);
    float v[C];
    sample_plane<C>(arena + desc.off[s][ci], W, t, v);
#pragma unroll
    for (int k = 0; k < C; ++k) prod[k] = j == 0 ? v[k] : prod[k] * v[k];
  }
}

template <int C>
__device__ __forceinline__ void group_adjoint(const PlaneDesc& desc, const float* __restrict__ arena, float* __restrict__ garena, int s,
                                              bool time_group, const Group<C>& g, const float gprod[C], bool want_coord,
                                              float gcoord[4]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int ci = group_plane(time_group, j);
    const int a = COMB_A[ci], b = COMB_B[ci];
    // product rule: d(prod)/d(v_j) = product of the other two planes of the group
    float gv[C];
    bool any = false;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      float other = 1.0f;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i != j) other *= g.v[i][k];
      gv[k] = gprod[k] * other;
      any |= gv[k] != 0.0f;
    }
    if (!any) continue;
    float gix = 0.0f, giy = 0.0f;
    scatter_plane<C>(garena + desc.off[s][ci], arena + desc.off[s][ci], desc.res[s][a], g.taps[j], gv, gix, giy, want_coord);
    gcoord[a] += gix * g.taps[j].mx;
    gcoord[b] += giy * g.taps[j].my;
  }
}

// dxt adds a coordinate's contributions group by group: static planes first, then time planes
template <int C>
__global__ void __launch_bounds__(256) planes_bwd_kernel(PlaneDesc desc, const float* __restrict__ arena,
                                                        const float* __restrict__ xt, int64_t P, int which,
                                                        const float* __restrict__ dout_s,
                                                        const float* __restrict__ dout_d, float* __restrict__ garena,
                                                        float* __restrict__ dxt) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float4_t c4 = *reinterpret_cast<const float4_t*>(xt + p * 4);
  const float coord[4] = {c4[0], c4[1], c4[2], c4[3]};
  const int n_out = desc.n_scales * C;
  float gcoord[4] = {0.f, 0.f, 0.f, 0.f};
  const bool want_coord = dxt != nullptr;
  for (int s = 0; s < desc.n_scales; ++s) {
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {  // 0: static, 1: time
      if ((which == 1 && grp == 1) || (which == 2 && grp == 0)) continue;
      const float* dout = grp ? dout_d : dout_s;
      Group<C> g;
      float prod[C], gp[C];
      group_sample<C>(desc, arena, s, grp == 1, coord, g, prod);
#pragma unroll
      for (int k = 0; k < C; ++k) gp[k] = dout ? dout[p * n_out + s * C + k] : 0.0f;
      group_adjoint<C>(desc, arena, garena, s, grp == 1, g, gp, want_coord, gcoord);
    }
  }
  if (want_coord) *reinterpret_cast<float4_t*>(dxt + p * 4) = float4_t{gcoord[0], gcoord[1], gcoord[2], gcoord[3]};
}

// the caller's arrays into a PlaneDesc; anything the kernels cannot index (a width other than 4, 8, 16, n_scales outside 1 .. 8, a null
// array, a resolution below 1) is refused, and `where` is the one text for all of these refusals
static int fill_desc(PlaneDesc& d, const int64_t* plane_off, const int32_t* res, int n_scales, int C, const char* where) {
  if (C != 4 && C != 8 && C != 16) {
    l4d_set_error(1, where);
    return 1;
  }
  if (n_scales < 1 || n_scales > MAX_SCALES || !plane_off || !res) {
    l4d_set_error(1, where);
    return 1;
  }
  d.n_scales = n_scales;
  for (int s = 0; s < n_scales; ++s) {
    for (int k = 0; k < 4; ++k) {
      if (res[s * 4 + k] < 1) {
        l4d_set_error(1, where);
        return 1;
      }
      d.res[s][k] = res[s * 4 + k];
    }
    for (int c = 0; c < NPLANES; ++c) d.off[s][c] = plane_off[s * NPLANES + c];
  }
  return 0;
}
