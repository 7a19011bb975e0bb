/*
 * lidar4d_patch.h -- C ABI of the patch depth-gradient loss (gfx950 / CDNA4): liblidar4d_patch.so.
 *
 * In its patch epochs the reference draws its rays as px x py pixel blocks of the range image and adds structure terms on
 * the depth patches to the training loss (model/runner.py:277-369; `--change_patch_size_lidar`, default [2, 8], every second
 * epoch).  Here the value of those terms and their gradient wrt the predicted depths come out of ONE sweep over the patches,
 * and the backward is the scaling of that gradient by the upstream one.  A library of its own, next to liblidar4d_hip.so
 * (include/lidar4d_hip.h), liblidar4d_prep.so (include/lidar4d_prep.h), liblidar4d_eval.so (include/lidar4d_eval.h) and
 * liblidar4d_loss.so (include/lidar4d_loss.h): loaded on first use, and the other libraries' ABIs stay what they are.
 *
 * Conventions as in lidar4d_loss.h: every pointer is a DEVICE pointer; tensors are dense; `stream` is a hipStream_t passed as
 * void*, last; outputs and workspaces are allocated by the caller and may arrive uninitialised; every entry point returns 0
 * on success or a hipError_t value (l4dg_last_error() gives the text); `*_workspace` return bytes.  No entry point
 * synchronises with the host, none calls memset, none uses floating-point atomics: the same input gives the same bits.
 *
 * The term, for predicted depths pred, measured depths gt and the ray-drop mask hit, each [n_patch, px, py] in ray order
 * (patch-major, then the px rows of a patch, then its py columns; "x" runs along a row, "y" down a column), pred and gt
 * already masked by the ray-drop -- exactly what lidar4d_amd.trainer.depth_grad_loss computes, quirks included:
 *   p = pred * (1.0f / scale),  q = gt * (1.0f / scale)        metres.  The restatement writes `x / scale` with a python float, which
 *                                                              torch evaluates on the device as this product, not as a quotient --
 *                                                              forward, and in autograd's backward (d pred = d p * (1.0f / scale))
 *   forward differences (default):
 *     rx(i,j) = p(i,j) - p(i,j+1)  [px, py-1],  ry(i,j) = p(i,j) - p(i+1,j)  [px-1, py]
 *     pgx = |rx|,  pgy = |ry|                                  the prediction side takes magnitudes ...
 *     ggx(i,j) = q(i,j) - q(i,j+1)                             ... the ground-truth side stays signed
 *     mask = hit(i,j) * (|ggx| < 0.01f)                        the left pixel's hit
 *   L4DG_SOBEL:
 *     pgx, pgy, ggx = 3 x 3 cross-correlation with [[-1,0,1],[-2,0,2],[-1,0,1]] (x) and its transpose (y), zero padding
 *     inside each patch, signed, [px, py];  mask = hit * (|ggx| < 0.01f)
 *   dx = |pgx|,  dy = |pgy|;  every mean runs over all elements of all patches of that difference image
 *   L4DG_GRAD_NORM_SMOOTH:  alpha_grad_norm * (mean exp(-dx) + mean exp(-dy))          accurate expf
 *   L4DG_SPATIAL_SMOOTH:    alpha_spatial   * (mean dx^2 + mean dy^2)
 *   L4DG_TV_LOSS:           alpha_tv        * (mean dx + mean dy)
 *   L4DG_GRAD_LOSS:         alpha_grad * sum term(a, b),  a = pgx * mask,  b = ggx * mask  (only the x direction, as the
 *                           reference has it), with
 *     L4DG_L1     |a - b|
 *     L4DG_MSE    (a - b)^2
 *     L4DG_HUBER  z = |a - b|, delta = (float)(0.2 * scale):  z < delta ? 0.5f * z * z : delta * (z - 0.5f * delta)
 *     L4DG_COS    per patch: 1 - sum (a / max(|a|_2, 1e-8)) * (b / max(|b|_2, 1e-8));  a patch whose mask is all zero
 *                 contributes 1 and no gradient
 *   gradients are what autograd gives these expressions: abs and |a - b| have gradient 0 at 0, the Huber gradient is a - b
 *   below delta and +-delta from it on, a norm that the 1e-8 floor replaces passes no gradient.
 * fp32 discipline: every element-wise value is produced by the same fp32 operations in the same order (no contraction), so
 * that every branch decision -- mask, sign, Huber branch -- is the one torch takes; only the SUMS differ: fp64 here
 * (per-workgroup partials, added by one workgroup in a fixed order), fp32 trees in torch.
 * fp16 ground truth (gt_half != 0: gt and hit are both fp16, forward differences only) follows torch's half arithmetic:
 *   q = half((float)gt * (1.0f / scale)),  ggx = half(q(i,j) - q(i,j+1)),  mask = half(hit * (|ggx| < 0.01)),  b = half(ggx * mask),
 *   each widened to fp32 where it meets the prediction side.  (No half value lies between 0.01 and half(0.01): the
 *   comparison gives the same mask in either format.)
 */
#ifndef LIDAR4D_PATCH_H
#define LIDAR4D_PATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DG_ABI_VERSION 1

/* limits of a patch: 2 <= px, 2 <= py, px * py <= L4DG_MAX_PATCH_PIXELS */
#define L4DG_MAX_PATCH_PIXELS 1024

/* kind */
#define L4DG_L1 0
#define L4DG_MSE 1
#define L4DG_HUBER 2
#define L4DG_COS 3

/* flags */
#define L4DG_SOBEL 1
#define L4DG_GRAD_LOSS 2
#define L4DG_GRAD_NORM_SMOOTH 4
#define L4DG_SPATIAL_SMOOTH 8
#define L4DG_TV_LOSS 16

int l4dg_version(void);
const char* l4dg_last_error(void);

/* Bytes of workspace for l4dg_patch_fwd (a multiple of 8, independent of the shape: the partials of a bounded grid); 0 for
 * a shape it rejects (n_patch < 1, px < 2, py < 2, px * py > L4DG_MAX_PATCH_PIXELS, or 2^31 pixels and more in all). */
int64_t l4dg_patch_workspace(int32_t n_patch, int32_t px, int32_t py);

/* Value and gradient of the term.  pred [n_patch * px * py] fp32; gt, hit: the same shape, both fp16 if gt_half != 0, else
 * both fp32 (not read, and may be null, without L4DG_GRAD_LOSS); kind: L4DG_L1 ... L4DG_COS; flags: the bits above.
 * loss_out [1] fp32: the value.  g_pred_out [n_patch * px * py] fp32: d loss / d pred for an upstream gradient of 1; every
 * element is written, with plain stores.  Two launches: one sweep over the patches that writes the gradient and one fp64
 * partial per workgroup -- a patch is reduced inside one wavefront while px * py <= 64, inside one workgroup beyond; every
 * pixel GATHERS the differences or stencil taps it takes part in -- then one workgroup that adds the partials in a fixed order.
 * workspace: l4dg_patch_workspace(n_patch, px, py) bytes, 8-byte aligned; its contents need not be initialised and are not
 * kept. */
int l4dg_patch_fwd(const float* pred, const void* gt, const void* hit, int32_t gt_half, int32_t n_patch, int32_t px,
                   int32_t py, float scale, int32_t kind, int32_t flags, float alpha_grad, float alpha_grad_norm,
                   float alpha_spatial, float alpha_tv, float* loss_out, float* g_pred_out, void* workspace, void* stream);

/* d_pred_out[i] = g[0] * g_pred[i], i < n: the gradient l4dg_patch_fwd left, scaled by the upstream gradient of the scalar
 * loss (g [1] fp32 on the device, loss scale included).  One launch; every element is written, with plain stores. */
int l4dg_patch_bwd(const float* g_pred, const float* g, int64_t n, float* d_pred_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_PATCH_H */
