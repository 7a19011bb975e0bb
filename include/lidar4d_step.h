/*
 * lidar4d_step.h -- C ABI of the two ends of a training step on a real sequence (gfx950 / CDNA4): liblidar4d_step.so.
 *
 * The reference preloads a sequence's ground truth as fp16 (data/kitti360_dataset.py:141-147), draws a step's rays as pixels or
 * px x py pixel patches of one frame (data/base_dataset.py:36-102) and evaluates the three primary losses with any of four
 * criteria each (main_lidar4d.py:63-66, model/runner.py:179-213).  These two entry points are the only ray batch and the only
 * primary losses the project has: every dataset and every criterion set goes through them, the benchmarked fp32 / single-pixel /
 * l1-mse-mse step included.  A library of its own, next to liblidar4d_prep.so, liblidar4d_eval.so, liblidar4d_loss.so and
 * liblidar4d_patch.so: loaded on first use.
 *
 * Conventions as in lidar4d_loss.h: every pointer is a DEVICE pointer; tensors are dense; `stream` is a hipStream_t passed as
 * void*, last; outputs and workspaces are allocated by the caller and may arrive uninitialised; every entry point returns 0
 * on success or a hipError_t value (l4ds_last_error() gives the text); `*_workspace` return bytes.  No entry point
 * synchronises with the host, none calls memset, none uses floating-point atomics: the same input gives the same bits.
 *
 * fp32 discipline: the element-wise arithmetic is written in the reference's operation order and compiled without
 * contraction, and the loss is summed in a fixed order (csrc/glue_dev.h), so that a numpy float32 evaluation in the same order
 * gives the bits of l4ds_primary_losses for L4DS_L1 depth, L4DS_MSE ray-drop and L4DS_MSE intensity on fp32 ground truth
 * (tests/realdata_cases.py primary_losses_ref).
 */
#ifndef LIDAR4D_STEP_H
#define LIDAR4D_STEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DS_ABI_VERSION 1

/* criterion of one loss term (--depth_loss / --raydrop_loss / --intensity_loss), reduction none:
 *   L4DS_L1     |a - b|
 *   L4DS_MSE    (a - b)^2
 *   L4DS_BCE    binary cross entropy with logits: (1 - b) * a - log_sigmoid(a)
 *   L4DS_HUBER  z = |a - b|:  z < delta ? 0.5f * z * z : delta * (z - 0.5f * delta) */
#define L4DS_L1 0
#define L4DS_MSE 1
#define L4DS_BCE 2
#define L4DS_HUBER 3

int l4ds_version(void);
const char* l4ds_last_error(void);

/* One frame's ray batch from n_patch drawn patch corners: top, left [n_patch] int64, patch shape px x py (1 x 1: single pixels).
 * Ray k = (patch * px + r) * py + c (patch-row major) looks through row top[patch] + r, column (left[patch] + c) mod W:
 *   inds [n] int64 = row * W + column;  rays_o, rays_d [n, 3] fp32 for pose [4, 4] fp32 (sensor to world, row major) and the
 *   field of view (fov_up, fov) in degrees, as data/base_dataset.py:82-102;
 *   gt [n, 3]: the three channels of the pixel in the FRAME'S OWN type -- image [H, W, 3] and gt are both fp16 if
 *   image_half != 0, else both fp32; half stays half.  image may be null (then gt is not written).
 * n = n_patch * px * py below 2^31.  A row outside [0, H) (no draw of the reference's produces one) reads no pixel: its gt is 0.
 * One launch; n_patch == 0 is a valid call that launches nothing. */
int l4ds_ray_batch(const int64_t* top, const int64_t* left, int32_t n_patch, int32_t px, int32_t py, const float* pose,
                   float fov_up, float fov, int32_t H, int32_t W, const void* image, int32_t image_half, float* rays_o,
                   float* rays_d, void* gt, int64_t* inds, void* stream);

/* Bytes of workspace for l4ds_primary_losses over n rays (one fp32 partial per workgroup of 256 rays, at least one); 0 for n < 0. */
int64_t l4ds_primary_losses_workspace(int32_t n);

/* The sum of model/runner.py:179-213 over n rays and its gradients.  depth [n], image [n, 2] (ray-drop, intensity) fp32: the
 * render outputs; gt [n, 3] (ray-drop mask m, intensity, depth): fp16 if gt_half != 0, else fp32.
 *   gt_i = gt[1] * m, gt_d = gt[2] * m, gs = clamp(m, smooth, 1 - smooth): for fp16 ground truth these three are taken in half as
 *   torch takes them (fp32 arithmetic, the result rounded to half; the bounds are half(smooth) and half(1.0f - smooth), so the
 *   smoothing targets of 0.2 are 0.199951171875 and 0.7998046875) -- everything after them is fp32 on the exactly widened values;
 *   p_i = image[1] * m, p_d = depth * m, p_r = image[0], or sigmoid(image[0]) when kind_raydrop is L4DS_BCE (runner.py:197-198);
 *   loss = sum over rays of alpha_d * crit_depth(p_d, gt_d) + alpha_r * crit_raydrop(p_r, gs) + alpha_i * crit_intensity(p_i, gt_i),
 *   delta: L4DS_HUBER's (the caller passes 0.2 * scale).
 * loss_out [1]; g_depth_out [n] = d loss / d depth; g_image_out [n, 2] = d loss / d image: what autograd gives the expressions
 * above (|x| has gradient 0 at 0).  Optional, null to skip:
 *   pts_out [2, n, 3]: rays_d * p_d / scale and rays_d * gt_d / scale, the two point sets of the ray-chamfer term
 *   (runner.py:216-217; rays_d [n, 3] fp32 is read only for them);
 *   gt32_out [n, 3]: gt widened to fp32.
 * Two launches: one workgroup of 256 threads per 256 rays writes the gradients and its partial sum, then one workgroup adds the
 * partials in index order.  n == 0 is a valid call: it writes loss_out[0] = 0 and nothing else.
 * workspace: l4ds_primary_losses_workspace(n) bytes, 4-byte aligned, not initialised, not kept. */
int l4ds_primary_losses(const float* depth, const float* image, const void* gt, int32_t gt_half, const float* rays_d, int32_t n,
                        int32_t kind_depth, int32_t kind_raydrop, int32_t kind_intensity, float alpha_d, float alpha_r,
                        float alpha_i, float smooth, float delta, float scale, float* loss_out, float* g_depth_out,
                        float* g_image_out, float* pts_out, float* gt32_out, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_STEP_H */
