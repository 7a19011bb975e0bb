/*
 * lidar4d_mlp.h -- C ABI of the width-generic fused MLP (gfx950 / CDNA4): liblidar4d_mlp.so.
 *
 * The reference exposes --hidden_dim_sigma / --hidden_dim_lidar / --hidden_dim_flow (main_lidar4d.py:53-59), and tiny-cuda-nn's
 * FullyFusedMLP accepts 16, 32, 64 and 128 neurons.  liblidar4d_hip.so (include/lidar4d_hip.h: l4d_mlp_fwd, l4d_mlp_fwd_sigma,
 * l4d_mlp_bwd) has the kernels of width 64, tuned for the default model, which stay what they are; this library has the same
 * network for the hidden widths 16, 32 and 128.  A library of its own, next to liblidar4d_prep.so, liblidar4d_eval.so,
 * liblidar4d_loss.so, liblidar4d_patch.so and liblidar4d_step.so: loaded on first use (a model of width 64 never maps it), and the
 * other libraries' ABIs stay what they are.
 *
 * The network: bias-free, ReLU hidden layers, no output activation; fp16 operands, fp32 accumulation on the matrix cores; the
 * input is in_pad columns wide (padding supplied by the caller), the output padded to 16.
 *   weights (fp16, row major, concatenated): W1 [hidden, in_pad], (n_hidden - 1) x [hidden, hidden], Wo [16, hidden]
 *   -- the layout of l4d_mlp_fwd with 64 replaced by hidden.
 * Shapes: hidden in {16, 32, 128}; in_pad in {16, 32, 64, 96, 128, 160, 176, 192}; n_hidden in {1, 2, 3}.  Anything else, hidden = 64
 * included, is refused with status 1.
 *
 * Conventions as in lidar4d_step.h: every pointer is a DEVICE pointer; tensors are dense; `stream` is a hipStream_t passed as
 * void*, last; outputs are allocated by the caller and may arrive uninitialised (grad_w excepted: it is added to); every entry
 * point returns 0 on success or a hipError_t value (l4dm_last_error() gives the text).  No entry point synchronises with the host
 * and none calls memset.
 *
 * Rows: `cap` is the row count the buffers were sized for (and the stride of the activation planes); n_rows, if not null, is a
 * device int32: the rows present are min(*n_rows, cap).  Rows at or past that count are neither read nor written.
 */
#ifndef LIDAR4D_MLP_H
#define LIDAR4D_MLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DM_ABI_VERSION 1

int l4dm_version(void);
const char* l4dm_last_error(void);

/* Forward.  x [cap, in_pad] fp16 -> y [cap, 16] fp16: the fp32 accumulator clamped to the fp16 range and rounded to nearest even,
 * as l4d_mlp_fwd stores it.  Optional, null to skip:
 *   act   [n_hidden, cap, hidden] fp16: the hidden layers' ReLU outputs (what l4dm_mlp_bwd reads);
 *   sigma [cap] fp32 = exp(fp16 y[row][0]): the density activation (trunc_exp's forward) as epilogue, as l4d_mlp_fwd_sigma.
 * One launch; cap == 0 is a valid call that launches nothing. */
int l4dm_mlp_fwd(const void* x, int64_t cap, const int32_t* n_rows, int32_t in_pad, int32_t hidden, int32_t n_hidden,
                 const void* weights, void* y, void* act, float* sigma, void* stream);

/* Backward, the contract of l4d_mlp_bwd.  x [cap, in_pad], act [n_hidden, cap, hidden] (required: the hidden activations are not
 * recomputed), dy [cap, 16], all fp16.
 *   grad_w (fp32, the weights' layout) += inv_scale * dW    -- ACCUMULATED with fp32 atomics, not overwritten;
 *   dx [cap, in_pad] fp16, null to skip.
 * The ReLU gate is act > 0.  dZ of every layer and dx are rounded to fp16 (nearest even) and NOT saturated: an overflow becomes
 * inf and reaches the caller's loss scaler.
 * dx_absmax, if not null (needs dx): *dx_absmax = max(*dx_absmax, max |dx[:, absmax_lo : absmax_hi]|) over the rows present, of
 * the values as stored, +inf if one of them is not finite; absmax_lo / absmax_hi are multiples of 16 inside [0, in_pad].
 * One launch for hidden 16 and 32; two for hidden 128 (the weight gradients, then dx). */
int l4dm_mlp_bwd(const void* x, const void* act, const void* dy, int64_t cap, const int32_t* n_rows, int32_t in_pad,
                 int32_t hidden, int32_t n_hidden, const void* weights, void* dx, float* grad_w, float inv_scale,
                 float* dx_absmax, int32_t absmax_lo, int32_t absmax_hi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_MLP_H */
