// Hex-plane sampling for the channel counts 4, 8 and 16 (main_lidar4d.py --n_features_per_level_plane): liblidar4d_planes.so,
// include/lidar4d_planes.h.  Width 8 stays in fused.hip / field_bwd.hip, tuned for the default model; this file is the same device
// functions (planes_dev.h, as they are) instantiated on the width, one thread per sample, plane gradients through global fp32
// atomics, and is not tuned:
//   * planes_fwd_kernel / planes_bwd_kernel are the templates of planes_kernels.h, the ones planes.hip launches at C = 8;
//   * density_planes_fwd_kernel / _bwd_kernel are the plane half of LiDAR4D.density (lidar4d.py:155-176) -- the static product at x,
//     the time product at (x, t0), (x + forward flow, t1), (x + backward flow, t2), the blend 0.5 d0 + 0.25 (d1 + d2) with a missing
//     neighbour replaced by d0 -- and its adjoint towards the planes, the flow and the coordinates.
// Indices: axis_tap clamps every texel index into its plane (a NaN or far-out-of-range warped coordinate lands on texel 0), W is the
// first axis of a pair and H the second (for time planes H is the time resolution), sample offsets are int64.
#include "common.h"

#include "planes_kernels.h"

#include "../../include/lidar4d_planes.h"

static_assert(L4DH_MAX_SCALES == MAX_SCALES, "the header's scale limit is planes_dev.h's");

extern "C" int l4dh_version(void) { return L4DH_ABI_VERSION; }
extern "C" const char* l4dh_last_error(void) { return l4d_last_error(); }

// the six flow columns of sample p (forward xyz, backward xyz), fp16 or fp32 rows of `stride` elements
__device__ __forceinline__ void load_flow(const void* __restrict__ flow, int stride, int is_half, int64_t p, float fl[6]) {
  if (is_half) {
    const half_t* f = reinterpret_cast<const half_t*>(flow) + p * stride;
#pragma unroll
    for (int k = 0; k < 6; ++k) fl[k] = h2f(f[k]);
  } else {
    const float* f = reinterpret_cast<const float*>(flow) + p * stride;
#pragma unroll
    for (int k = 0; k < 6; ++k) fl[k] = f[k];
  }
}

template <int C>
__global__ void __launch_bounds__(256) density_planes_fwd_kernel(PlaneDesc desc, const float* __restrict__ arena,
                                                                const float* __restrict__ xt, const void* __restrict__ flow,
                                                                int flow_stride, int flow_half, const float* __restrict__ tinfo,
                                                                int64_t P, float* __restrict__ out_s, float* __restrict__ out_d) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float4_t c4 = *reinterpret_cast<const float4_t*>(xt + p * 4);
  const float t0 = tinfo[0], t1 = tinfo[1], t2 = tinfo[2];
  const bool has_fwd = tinfo[3] != 0.0f, has_bwd = tinfo[4] != 0.0f;
  float fl[6];
  load_flow(flow, flow_stride, flow_half, p, fl);
  const float x0[4] = {c4[0], c4[1], c4[2], t0};
  const float x1[4] = {c4[0] + fl[0], c4[1] + fl[1], c4[2] + fl[2], t1};
  const float x2[4] = {c4[0] + fl[3], c4[1] + fl[4], c4[2] + fl[5], t2};
  const int n_out = desc.n_scales * C;
  for (int s = 0; s < desc.n_scales; ++s) {
    float ps[C], d0[C], d1[C], d2[C], pd[C];
    group_product<C>(desc, arena, s, false, x0, ps);
    group_product<C>(desc, arena, s, true, x0, d0);
    if (has_fwd) group_product<C>(desc, arena, s, true, x1, d1);
    if (has_bwd) group_product<C>(desc, arena, s, true, x2, d2);
#pragma unroll
    for (int k = 0; k < C; ++k) pd[k] = 0.5f * d0[k] + 0.25f * ((has_fwd ? d1[k] : d0[k]) + (has_bwd ? d2[k] : d0[k]));
    float4_t* os = reinterpret_cast<float4_t*>(out_s + p * n_out + s * C);
    float4_t* od = reinterpret_cast<float4_t*>(out_d + p * n_out + s * C);
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
      os[q] = float4_t{ps[q * 4], ps[q * 4 + 1], ps[q * 4 + 2], ps[q * 4 + 3]};
      od[q] = float4_t{pd[q * 4], pd[q * 4 + 1], pd[q * 4 + 2], pd[q * 4 + 3]};
    }
  }
}

template <int C>
__global__ void __launch_bounds__(256) density_planes_bwd_kernel(PlaneDesc desc, const float* __restrict__ arena,
                                                                const float* __restrict__ xt, const void* __restrict__ flow,
                                                                int flow_stride, int flow_half, const float* __restrict__ tinfo,
                                                                int64_t P, const float* __restrict__ d_out_s,
                                                                const float* __restrict__ d_out_d, float* __restrict__ garena,
                                                                float* __restrict__ dflow, float* __restrict__ dxt) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float4_t c4 = *reinterpret_cast<const float4_t*>(xt + p * 4);
  const float t0 = tinfo[0], t1 = tinfo[1], t2 = tinfo[2];
  const bool has_fwd = tinfo[3] != 0.0f, has_bwd = tinfo[4] != 0.0f;
  float fl[6];
  load_flow(flow, flow_stride, flow_half, p, fl);
  const float x0[4] = {c4[0], c4[1], c4[2], t0};
  const float x1[4] = {c4[0] + fl[0], c4[1] + fl[1], c4[2] + fl[2], t1};
  const float x2[4] = {c4[0] + fl[3], c4[1] + fl[4], c4[2] + fl[5], t2};
  // d(out_d)/d(d0): a missing neighbour's quarter goes to the frame's own lookup
  const float c0 = 0.5f + (has_fwd ? 0.0f : 0.25f) + (has_bwd ? 0.0f : 0.25f);
  const int n_out = desc.n_scales * C;
  const bool want_x = dxt != nullptr, want_f = dflow != nullptr;
  float g0[4] = {0.f, 0.f, 0.f, 0.f}, g1[4] = {0.f, 0.f, 0.f, 0.f}, g2[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < desc.n_scales; ++s) {
    float gs[C], gd[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
      gs[k] = d_out_s[p * n_out + s * C + k];
      gd[k] = d_out_d[p * n_out + s * C + k];
    }
    Group<C> g;
    float prod[C], ge[C];
    group_sample<C>(desc, arena, s, false, x0, g, prod);
    group_adjoint<C>(desc, arena, garena, s, false, g, gs, want_x, g0);
    group_sample<C>(desc, arena, s, true, x0, g, prod);
#pragma unroll
    for (int k = 0; k < C; ++k) ge[k] = c0 * gd[k];
    group_adjoint<C>(desc, arena, garena, s, true, g, ge, want_x, g0);
#pragma unroll
    for (int k = 0; k < C; ++k) ge[k] = 0.25f * gd[k];
    if (has_fwd) {
      group_sample<C>(desc, arena, s, true, x1, g, prod);
      group_adjoint<C>(desc, arena, garena, s, true, g, ge, want_x || want_f, g1);
    }
    if (has_bwd) {
      group_sample<C>(desc, arena, s, true, x2, g, prod);
      group_adjoint<C>(desc, arena, garena, s, true, g, ge, want_x || want_f, g2);
    }
  }
  if (want_f) {
    float* o = dflow + p * 6;
    o[0] = g1[0], o[1] = g1[1], o[2] = g1[2];
    o[3] = g2[0], o[4] = g2[1], o[5] = g2[2];
  }
  // x1 = x + forward flow, x2 = x + backward flow: the warped lookups' spatial gradients reach x as they are; t1 and t2 are constants
  if (want_x) *reinterpret_cast<float4_t*>(dxt + p * 4) = float4_t{g0[0] + g1[0] + g2[0], g0[1] + g1[1] + g2[1], g0[2] + g1[2] + g2[2], g0[3]};
}

// the launch of KERNEL<C> for the run-time C (fill_desc has refused anything but 4, 8, 16)
#define PLANES_WIDTH_LAUNCH(KERNEL, C, ...)                                                                          \
  do {                                                                                                               \
    const dim3 grid__((unsigned)ceil_div64(P, 256));                                                                 \
    if ((C) == 4) L4D_LAUNCH((KERNEL<4>), grid__, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                    \
    else if ((C) == 8) L4D_LAUNCH((KERNEL<8>), grid__, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);               \
    else L4D_LAUNCH((KERNEL<16>), grid__, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                            \
  } while (0)

extern "C" int l4dh_planes_fwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales, int32_t C,
                               const float* xt, int64_t P, int32_t which, float* out_s, float* out_d, void* stream) {
  if (P == 0) return 0;
  PlaneDesc d;
  if (fill_desc(d, plane_off, res, n_scales, C, "l4dh_planes_fwd: C must be 4, 8 or 16 and n_scales 1 .. 8 (positive resolutions)")) return 1;
  if (P < 0 || which < 0 || which > 2) L4D_FAIL("l4dh_planes_fwd: P < 0 or which outside 0 .. 2");
  if (!planes_cl || !xt || (which != 2 && !out_s) || (which != 1 && !out_d)) L4D_FAIL("l4dh_planes_fwd: planes_cl, xt and the outputs `which` asks for are required");
  PLANES_WIDTH_LAUNCH(planes_fwd_kernel, C, d, planes_cl, xt, P, which, out_s, out_d);
  L4D_LAUNCH_CHECK("l4dh_planes_fwd");
  return 0;
}

extern "C" int l4dh_planes_bwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales, int32_t C,
                               const float* xt, int64_t P, int32_t which, const float* dout_s, const float* dout_d, float* grad_cl,
                               float* dxt, void* stream) {
  if (P == 0) return 0;
  PlaneDesc d;
  if (fill_desc(d, plane_off, res, n_scales, C, "l4dh_planes_bwd: C must be 4, 8 or 16 and n_scales 1 .. 8 (positive resolutions)")) return 1;
  if (P < 0 || which < 0 || which > 2) L4D_FAIL("l4dh_planes_bwd: P < 0 or which outside 0 .. 2");
  if (!planes_cl || !xt || !grad_cl) L4D_FAIL("l4dh_planes_bwd: planes_cl, xt and grad_cl are required");
  PLANES_WIDTH_LAUNCH(planes_bwd_kernel, C, d, planes_cl, xt, P, which, dout_s, dout_d, grad_cl, dxt);
  L4D_LAUNCH_CHECK("l4dh_planes_bwd");
  return 0;
}

extern "C" int l4dh_density_planes_fwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales,
                                       int32_t C, const float* xt, const void* flow, int32_t flow_stride, int32_t flow_half,
                                       const float* tinfo, int64_t P, float* out_s, float* out_d, void* stream) {
  if (P == 0) return 0;
  PlaneDesc d;
  if (fill_desc(d, plane_off, res, n_scales, C, "l4dh_density_planes_fwd: C must be 4, 8 or 16 and n_scales 1 .. 8 (positive resolutions)")) return 1;
  if (P < 0 || flow_stride < 6) L4D_FAIL("l4dh_density_planes_fwd: P < 0 or a flow row of fewer than 6 columns");
  if (!planes_cl || !xt || !flow || !tinfo || !out_s || !out_d) L4D_FAIL("l4dh_density_planes_fwd: planes_cl, xt, flow, tinfo, out_s and out_d are required");
  PLANES_WIDTH_LAUNCH(density_planes_fwd_kernel, C, d, planes_cl, xt, flow, (int)flow_stride, (int)flow_half, tinfo, P, out_s, out_d);
  L4D_LAUNCH_CHECK("l4dh_density_planes_fwd");
  return 0;
}

extern "C" int l4dh_density_planes_bwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales,
                                       int32_t C, const float* xt, const void* flow, int32_t flow_stride, int32_t flow_half,
                                       const float* tinfo, int64_t P, const float* d_out_s, const float* d_out_d, float* grad_cl,
                                       float* dflow, float* dxt, void* stream) {
  if (P == 0) return 0;
  PlaneDesc d;
  if (fill_desc(d, plane_off, res, n_scales, C, "l4dh_density_planes_bwd: C must be 4, 8 or 16 and n_scales 1 .. 8 (positive resolutions)")) return 1;
  if (P < 0 || flow_stride < 6) L4D_FAIL("l4dh_density_planes_bwd: P < 0 or a flow row of fewer than 6 columns");
  if (!planes_cl || !xt || !flow || !tinfo || !d_out_s || !d_out_d || !grad_cl)
    L4D_FAIL("l4dh_density_planes_bwd: planes_cl, xt, flow, tinfo, d_out_s, d_out_d and grad_cl are required");
  PLANES_WIDTH_LAUNCH(density_planes_bwd_kernel, C, d, planes_cl, xt, flow, (int)flow_stride, (int)flow_half, tinfo, P, d_out_s,
                      d_out_d, grad_cl, dflow, dxt);
  L4D_LAUNCH_CHECK("l4dh_density_planes_bwd");
  return 0;
}
