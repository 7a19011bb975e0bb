// Hex-plane (K-Planes) feature sampling for gfx950, replacing the 24 F.grid_sample launches of
// model/planes_field.py:87-141 (bilinear, align_corners=True, border padding, product over the three
// static / three time planes of a scale, concat over scales) with one kernel, forward and backward
// (wrt planes AND wrt sample coordinates: the flow-warped neighbour-frame lookups of
// model/lidar4d.py:158-173 need d/dx).
//
// Layout: the [1,C,H,W] parameters are mirrored channel-last ([H,W,C], C=8 fp32 = 32 B per texel) so a
// bilinear tap is two 16-byte loads instead of 8 strided dwords; l4d_planes_relayout converts both ways
// (parameters -> compute copy, compute-layout gradients -> parameter-layout gradients).
// The two sampling kernels are the templates of planes_kernels.h at C = 8 (planes_width.hip launches them at 4, 8 and 16).
#include "common.h"

#include "planes_kernels.h"
#include <algorithm>

// [C,H,W] <-> [H,W,C], all planes of all scales in one launch (blockIdx.y = plane); mode 0: channel-last -> [C,H,W],
// 1: [C,H,W] -> channel-last, 2: channel-last ADDED onto [C,H,W] (gradients straight into the parameters' .grad views)
struct RelayoutPlanes {
  float* nchw[MAX_SCALES * NPLANES];
  int64_t off[MAX_SCALES * NPLANES];
  int H[MAX_SCALES * NPLANES], W[MAX_SCALES * NPLANES];
};
__global__ void __launch_bounds__(256) relayout_kernel(RelayoutPlanes pl, float* __restrict__ cl_base, int C, int mode) {
  const int k = blockIdx.y;
  const int H = pl.H[k], W = pl.W[k];
  const int64_t n = (int64_t)C * H * W;
  float* nchw = pl.nchw[k];
  float* cl = cl_base + pl.off[k];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (mode == 1) {  // i indexes cl [H,W,C]
      const int c = i % C;
      const int64_t hw = i / C;
      cl[i] = nchw[(int64_t)c * H * W + hw];
    } else {  // i indexes nchw [C,H,W]
      const int64_t hw = i % ((int64_t)H * W);
      const int c = i / ((int64_t)H * W);
      const float v = cl[hw * C + c];
      nchw[i] = mode == 2 ? nchw[i] + v : v;
    }
  }
}

extern "C" int l4d_planes_relayout(const float* const* planes, const int32_t* res, int32_t n_scales, int32_t C,
                                   float* planes_cl, const int64_t* plane_off, int32_t to_channel_last,
                                   void* stream) {
  if (n_scales > MAX_SCALES || to_channel_last < 0 || to_channel_last > 2) {
    l4d_set_error(1, "l4d_planes_relayout: too many scales / unknown mode");
    return 1;
  }
  RelayoutPlanes pl;
  int64_t max_n = 0;
  for (int s = 0; s < n_scales; ++s)
    for (int c = 0; c < NPLANES; ++c) {
      const int k = s * NPLANES + c;
      static const int CA[NPLANES] = {0, 0, 0, 1, 1, 2}, CB[NPLANES] = {1, 2, 3, 2, 3, 3};  // comb order of the six planes
      pl.W[k] = res[s * 4 + CA[c]];
      pl.H[k] = res[s * 4 + CB[c]];
      pl.off[k] = plane_off[k];
      pl.nchw[k] = const_cast<float*>(planes[k]);
      max_n = std::max<int64_t>(max_n, (int64_t)C * pl.H[k] * pl.W[k]);
    }
  if (max_n == 0) return 0;
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(max_n, 256), 512);
  L4D_LAUNCH(relayout_kernel, dim3(gx, n_scales * NPLANES), dim3(256), 0, (hipStream_t)stream, pl, planes_cl, C, to_channel_last);
  L4D_LAUNCH_CHECK("l4d_planes_relayout");
  return 0;
}

extern "C" int l4d_planes_fwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales,
                              int32_t C, const float* xt, int64_t P, int32_t which, float* out_s, float* out_d,
                              void* stream) {
  if (P == 0) return 0;
  if (C != 8) {
    l4d_set_error(1, "planes: C must be 8");
    return 1;
  }
  PlaneDesc d;
  if (fill_desc(d, plane_off, res, n_scales, C, "l4d_planes_fwd: n_scales must be 1 .. 8 (positive resolutions)")) return 1;
  L4D_LAUNCH((planes_fwd_kernel<8>), dim3((unsigned)ceil_div64(P, 256)), dim3(256), 0, (hipStream_t)stream, d,
                     planes_cl, xt, P, which, out_s, out_d);
  L4D_LAUNCH_CHECK("l4d_planes_fwd");
  return 0;
}

extern "C" int l4d_planes_bwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales,
                              int32_t C, const float* xt, int64_t P, int32_t which, const float* dout_s,
                              const float* dout_d, float* grad_cl, float* dxt, void* stream) {
  if (P == 0) return 0;
  if (C != 8) {
    l4d_set_error(1, "planes: C must be 8");
    return 1;
  }
  PlaneDesc d;
  if (fill_desc(d, plane_off, res, n_scales, C, "l4d_planes_bwd: n_scales must be 1 .. 8 (positive resolutions)")) return 1;
  L4D_LAUNCH((planes_bwd_kernel<8>), dim3((unsigned)ceil_div64(P, 256)), dim3(256), 0, (hipStream_t)stream, d,
                     planes_cl, xt, P, which, dout_s, dout_d, grad_cl, dxt);
  L4D_LAUNCH_CHECK("l4d_planes_bwd");
  return 0;
}
