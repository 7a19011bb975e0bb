/*
 * lidar4d_planes.h -- C ABI of the width-generic hex-plane sampler (gfx950 / CDNA4): liblidar4d_planes.so.
 *
 * The reference exposes --n_features_per_level_plane (main_lidar4d.py), the channel count C of every hex-plane.  liblidar4d_hip.so
 * (include/lidar4d_hip.h: l4d_planes_fwd / l4d_planes_bwd and the fused field encode) is built for C = 8, the default, and stays what
 * it is; this library has the plane sampler, and the plane half of LiDAR4D.density (lidar4d.py:155-176) as one launch each way, for
 * C in {4, 8, 16}.  C = 8 exists here so that these kernels can be compared with liblidar4d_hip.so's; the product path of C = 8 does not
 * use it.  A library of its own, next to liblidar4d_prep.so ... liblidar4d_mlp.so: loaded on first use, and the other libraries'
 * ABIs stay what they are.  The kernels are one thread per sample with global fp32 atomics for the plane gradients: they are not
 * tuned.
 *
 * The planes: l4d_planes_fwd's arena.  planes_cl is one fp32 DEVICE buffer holding every plane channel-last ([H, W, C]);
 * plane_off [n_scales * 6] (element offsets, int64) and res [n_scales * 4] (x, y, z, t resolution per scale) are HOST arrays;
 * the six planes of a scale come in the order (x,y) (x,z) (x,t) (y,z) (y,t) (z,t), the first axis of a pair is W, the second H.
 * l4d_planes_relayout (include/lidar4d_hip.h) takes C at run time and converts [1, C, H, W] parameters to and from this layout.
 * Sampling is ATen's grid_sampler_2d: bilinear, align_corners = True, border padding (planes_field.py:56-84).
 *
 * Conventions as in lidar4d_mlp.h: every pointer but plane_off / res is a DEVICE pointer; tensors are dense unless a stride is
 * given; `stream` is a hipStream_t passed as void*, last; outputs are allocated by the caller and may arrive uninitialised
 * (grad_cl excepted: it is added to); every entry point returns 0 on success or a hipError_t value (l4dh_last_error() gives the
 * text).  No entry point synchronises with the host and none calls memset.  P == 0 is a valid call that launches nothing;
 * C outside {4, 8, 16} or n_scales outside 1 .. 8 is refused with status 1.
 */
#ifndef LIDAR4D_PLANES_H
#define LIDAR4D_PLANES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DH_ABI_VERSION 1
#define L4DH_MAX_SCALES 8

int l4dh_version(void);
const char* l4dh_last_error(void);

/* The contract of l4d_planes_fwd.  xt [P, 4] fp32 -> out_s / out_d [P, n_scales * C] fp32, scale-major: per scale the product of the
 * three static planes (xy, xz, yz) / of the three time planes (xt, yt, zt).  which = 0: both; 1: out_s only (out_d is not touched);
 * 2: out_d only. */
int l4dh_planes_fwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales, int32_t C,
                    const float* xt, int64_t P, int32_t which, float* out_s, float* out_d, void* stream);

/* The contract of l4d_planes_bwd.  dout_s / dout_d [P, n_scales * C] fp32 (the one `which` leaves out is not read);
 * grad_cl (the arena's layout) += the plane gradients, fp32 atomics; dxt [P, 4] fp32 receives d/d(xt), null to skip. */
int l4dh_planes_bwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales, int32_t C,
                    const float* xt, int64_t P, int32_t which, const float* dout_s, const float* dout_d, float* grad_cl,
                    float* dxt, void* stream);

/* The plane half of LiDAR4D.density in one launch.  xt [P, 4] fp32 = (x, y, z, t0); flow: row p holds (forward xyz, backward xyz)
 * in its first six columns, fp16 if flow_half != 0 else fp32, flow_stride elements from one row to the next (>= 6);
 * tinfo: l4d_time_setup's floats (t0, t1, t2, has_fwd, has_bwd).
 *   out_s [P, n_scales * C] = product of the static planes at x
 *   out_d [P, n_scales * C] = 0.5 d0 + 0.25 (d1 + d2), d0 the product of the time planes at (x, t0), d1 at (x + forward flow, t1),
 *                             d2 at (x + backward flow, t2); a neighbour the frame does not have (has_fwd / has_bwd == 0) is d0. */
int l4dh_density_planes_fwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales, int32_t C,
                            const float* xt, const void* flow, int32_t flow_stride, int32_t flow_half, const float* tinfo,
                            int64_t P, float* out_s, float* out_d, void* stream);

/* Its adjoint from d_out_s / d_out_d [P, n_scales * C] fp32.  grad_cl += the plane gradients (fp32 atomics);
 * dflow [P, 6] fp32, null to skip: through the two warped time-plane lookups only, zero in the three columns of a missing neighbour;
 * dxt [P, 4] fp32, null to skip: d/d(x, y, z) through all lookups, d/d(t0) through the lookup at t0 (t1 and t2 are constants). */
int l4dh_density_planes_bwd(const float* planes_cl, const int64_t* plane_off, const int32_t* res, int32_t n_scales, int32_t C,
                            const float* xt, const void* flow, int32_t flow_stride, int32_t flow_half, const float* tinfo,
                            int64_t P, const float* d_out_s, const float* d_out_d, float* grad_cl, float* dflow, float* dxt,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_PLANES_H */
