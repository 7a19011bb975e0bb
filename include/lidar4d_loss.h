/*
 * lidar4d_loss.h -- C ABI of the line-of-sight loss (gfx950 / CDNA4): liblidar4d_loss.so.
 *
 * The reference's `--urf_loss` term (model/runner.py:255-276, the line-of-sight loss of Urban Radiance Fields) works on the two
 * largest tensors of a training step, the compositing weights and the sample depths, both [N,T].  Here its value and its
 * gradient wrt the weights are two entry points: a few sweeps over the two tensors, no [N,T] temporary, the tolerance's
 * schedule evaluated on the device, so that the term can be part of a captured step.  A library of its own, next to
 * liblidar4d_hip.so (include/lidar4d_hip.h), liblidar4d_prep.so (include/lidar4d_prep.h) and liblidar4d_eval.so
 * (include/lidar4d_eval.h): loaded on first use, and the render path's ABI stays what it is.
 *
 * Conventions as in lidar4d_hip.h: every pointer is a DEVICE pointer; tensors are dense row-major; `stream` is a hipStream_t
 * passed as void*; outputs and workspaces are allocated by the caller; every entry point returns 0 on success or a
 * hipError_t value (l4dl_last_error() gives the text); `*_workspace` return bytes.  No entry point synchronises with the host.
 *
 * The term, for weights w [N,T], sample depths z [N,T] and measured depths d [N] (0 = no return):
 *   it    = sched ? sched[0] : step                          (sched: device, [iterations so far, ...] of the optimiser)
 *   eps   = 0.02 * 0.1 ^ min(it / iters, 1)                  fp64, on the device in both cases
 *   lo    = d - (float)eps,  hi = d + (float)eps             fp32, no contraction; for fp16 depths rounded to fp16 and widened
 *                                                            (what torch's half_tensor - python_float gives)
 *   near  = z > lo && z < hi,  empty = z < lo || z > hi      strict: a sample exactly on a bound is neither
 *   x     = near ? z - d : 0,  sigma = eps / 3,  bell = exp(-(x * x) / (float)(2 sigma^2))    accurate expf
 *   m     = max of bell over ALL N * T samples               (1 as soon as one sample anywhere is not near; computed, not assumed)
 *   b     = near ? bell / m : 0
 *   n_hit = number of rays with d > 0
 *   loss  = 0.1 * sum((empty * w)^2) / n_hit + 0.1 * sum((near * w - b)^2) / n_hit
 *   d_weights = g * 0.2 / n_hit * (empty * w + near * (w - b))
 * Squares and differences in fp32 as torch takes them; the sums in fp64: per-workgroup partials, added up by one workgroup in
 * a fixed order.  No floating-point atomics: the same input gives the same bits.  n_hit = 0 divides as IEEE does.
 */
#ifndef LIDAR4D_LOSS_H
#define LIDAR4D_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DL_ABI_VERSION 1

int l4dl_version(void);
const char* l4dl_last_error(void);

/* Bytes of workspace for l4dl_los_fwd / l4dl_los_bwd on [N,T] tensors (a multiple of 8, independent of the shape: the
 * partials of a bounded grid); 0 for a shape they reject (N < 1 or T < 1). */
int64_t l4dl_los_workspace(int32_t N, int32_t T);

/* Value of the term.  weights, z_vals: [N,T] fp32; gt_depth: [N], fp16 if gt_half != 0, else fp32; sched: device pointer to
 * the optimiser's schedule state (sched[0] = iterations so far, fp32) or null, then `step` is used; iters >= 1.
 * loss_out [1] fp32.  Three launches: normaliser and n_hit (stops reading a ray's z_vals at its first sample that is not
 * near), the two sums (one sweep over both tensors), the result.
 * workspace: l4dl_los_workspace(N, T) bytes, 8-byte aligned; its contents need not be initialised and are not kept. */
int l4dl_los_fwd(const float* weights, const float* z_vals, const void* gt_depth, int32_t gt_half, int32_t N, int32_t T,
                 const float* sched, int32_t step, int32_t iters, float* loss_out, void* workspace, void* stream);

/* Gradient of the term wrt the weights.  Inputs as for l4dl_los_fwd (the call stands on its own: it needs nothing a forward
 * call left behind); g [1] fp32 on the device: the upstream gradient of the scalar loss, loss scale included.
 * d_weights [N,T] fp32: every element is written, with plain stores.  Two launches: normaliser and n_hit, then one sweep
 * that reads both tensors and writes the gradient.  workspace as above. */
int l4dl_los_bwd(const float* weights, const float* z_vals, const void* gt_depth, int32_t gt_half, int32_t N, int32_t T,
                 const float* sched, int32_t step, int32_t iters, const float* g, float* d_weights, void* workspace,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_LOSS_H */
