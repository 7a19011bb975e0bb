/*
 * lidar4d_eval.h -- C ABI of the evaluation meters' kernels (gfx950 / CDNA4): liblidar4d_eval.so.
 *
 * The reference scores every validation frame's rendered depth and intensity image against the ground truth with numpy and
 * skimage on the host (utils/metrics.py:64-86,135-157: clamp, RMSE, median absolute error, SSIM, PSNR).  Here the error
 * statistics of one image pair are one entry point on the device, so that nothing leaves the GPU until the meters'
 * measure().  A library of its own, next to liblidar4d_hip.so (include/lidar4d_hip.h) and liblidar4d_prep.so
 * (include/lidar4d_prep.h): evaluation work, loaded on first use, and the render path's ABI stays what it is.
 *
 * Conventions as in lidar4d_hip.h: every pointer is a DEVICE pointer; tensors are dense row-major; `stream` is a hipStream_t
 * passed as void*; outputs and workspaces are allocated by the caller; every entry point returns 0 on success or a
 * hipError_t value (l4de_last_error() gives the text); `*_workspace` return bytes.  No entry point synchronises with the host.
 */
#ifndef LIDAR4D_EVAL_H
#define LIDAR4D_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DE_ABI_VERSION 1
#define L4DE_SSIM_WINDOW 7 /* skimage.metrics.structural_similarity's default win_size */

int l4de_version(void);
const char* l4de_last_error(void);

/* Bytes of workspace for l4de_image_errors on an [H,W] image; 0 for a shape it rejects. */
int64_t l4de_image_errors_workspace(int32_t H, int32_t W);

/* Error statistics of one image pair.  pred, gt: [H,W] fp32, already divided by the meter's scale; lo, hi: clamp bounds.
 * out [4] fp64: rmse, medae, ssim, psnr.  H >= 7 and W >= 7 (one SSIM window), H * W <= 2^28; otherwise an error status.
 *   p = pred < lo ? lo : (pred > hi ? hi : pred), g likewise from gt (a NaN stays a NaN); d = g - p in fp32
 *   rmse  = sqrt(mean(d * d)), squares and sum in fp64;  psnr = 10 * log10(hi * hi / mean(d * d)) in fp64
 *   medae = median of the H * W fp32 values |d| by exact selection; for an even count (a + b) / 2 of the two middle values in
 *           fp32; NaN if any |d| is NaN
 *   ssim  = mean over the (H-6) x (W-6) windows inside the image of
 *           (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), 7x7 uniform window means, sample covariance
 *           (49/48), C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = max(g) - min(g); fp64 throughout (structural_similarity's defaults)
 * Every reduction has a fixed order: the same input gives the same bits.  workspace: l4de_image_errors_workspace(H, W) bytes,
 * 8-byte aligned; its contents need not be initialised and are not kept. */
int l4de_image_errors(const float* pred, const float* gt, int32_t H, int32_t W, float lo, float hi, double* out, void* workspace,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_EVAL_H */
