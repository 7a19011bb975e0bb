/*
 * lidar4d_march.h -- C ABI of the slab-by-slab ray march with early termination (gfx950 / CDNA4): liblidar4d_march.so.
 *
 * A no-grad render (Simulator.render, Trainer.evaluate / test_step / collect_refine_data) may ask for early_stop = eps: a ray's
 * samples are evaluated front to back in slabs of S samples, and a ray whose transmittance so far,
 *   T^ = prod_k ((1 - alpha_k) + 1e-15f),   alpha_k as l4d_composite_fwd forms it (include/lidar4d_hip.h),
 * has dropped below eps after a slab is RETIRED: its remaining samples are not evaluated and count as sigma = 0.  The field and the
 * networks of a slab run through liblidar4d_hip.so's entry points on COMPACT rows (live rays only); this library has the two
 * kernels around them and the start values.  Per slab (lidar4d_amd/early_stop.py):
 *   l4dr_slab_rows   -> the (x, y, z, t) rows of the live rays' samples s0 .. s0 + S' - 1
 *   (flow grid, flow network, field encode + density network: l4d_hashgrid_t_fwd, l4d_mlp_fwd, l4d_density_encode_sigma_fwd)
 *   l4dr_slab_update -> sigma / h rows to their dense places, T^, retirement, the next slab's live list in ascending ray order
 * and the host reads ONE int32, the number of live rays, to size the next slab's launches.  What follows (compositing, the attribute
 * networks, the image) is the plain render's, on the dense sigma that holds 0 behind every ray's retirement point.
 *
 * Conventions as in lidar4d_planes.h: every pointer is a DEVICE pointer; tensors are dense; `stream` is a hipStream_t passed as
 * void*, last; outputs are allocated by the caller and may arrive uninitialised (trans excepted: l4dr_march_init starts it, every
 * l4dr_slab_update multiplies it); every entry point returns 0 on success or a hipError_t value (l4dr_last_error() gives the text).
 * No entry point synchronises with the host, none calls memset and none uses a floating-point atomic: two calls on the same
 * inputs give the same bits in the same order.  N == 0 or n_live == 0 is a valid call that launches nothing and writes nothing.
 * T < 1, S < 1, s0 outside 0 .. T - 1, n_live > N or an eps that is negative or NaN is refused with status 1.
 *
 * S' = min(S, T - s0) is the number of samples of the slab that starts at s0; compact row i * S' + (s - s0) belongs to sample s
 * of ray live[i].
 */
#ifndef LIDAR4D_MARCH_H
#define LIDAR4D_MARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DR_ABI_VERSION 1

int l4dr_version(void);
const char* l4dr_last_error(void);

/* Start of a march over N rays: trans [N] fp32 = 1, live [N] int32 = 0 .. N - 1, *n_live (int32) = N. */
int l4dr_march_init(int64_t N, float* trans, int32_t* live, int32_t* n_live, void* stream);

/* xt_out [n_live * S', 4] fp32: for live ray live[i] (int32, 0 <= live[i] < N) and sample s of the slab, row i * S' + (s - s0) holds
 * the bits l4d_sample_rays_xt writes to row live[i] * T + s of its xt when it is given no noise: the clipped sample position mapped
 * to [0, 1]^3 and the time *t.  rays_o / rays_d [N, 3] fp32, lin [T] fp32 (torch.linspace(0, 1, T)), t: one fp32. */
int l4dr_slab_rows(const float* rays_o, const float* rays_d, const float* lin, const float* t, const int32_t* live, int64_t n_live,
                   int64_t N, int32_t T, int32_t s0, int32_t S, float near, float far, float bound, float* xt_out, void* stream);

/* Bytes of workspace l4dr_slab_update needs for n_live rays. */
int64_t l4dr_slab_update_workspace(int64_t n_live);

/* Behind the density network of a slab.  sigma_c [n_live * S'] fp32 and h_c [n_live * S', 16] fp16 are its outputs on the compact
 * rows; z_vals [N, T] fp32 the dense sample distances (l4d_sample_rays); sample_dist, density_scale, active_sensor as given to
 * l4d_composite_fwd.  Per live ray r = live[i], one wavefront:
 *   sigma_dense [N, T] fp32 and h_dense [N * T, 16] fp16 receive the slab's values at samples s0 .. s0 + S' - 1 of ray r;
 *   trans[r] *= the product of the slab's factors (1 - alpha) + 1e-15f: lane l multiplies the factors of samples s0 + l,
 *     s0 + l + 64, ... in that order, starting from the first; the 64 lane products are combined by a tree, v[l] = v[l] * v[l + o]
 *     for o = 32, 16, ... 1; trans[r] = trans[r] * v[0];
 *   the ray is retired if trans[r] < eps afterwards (a NaN compares false: never retired).  Then, unless this is the last slab
 *     (s0 + S >= T), sigma_dense of its samples s0 + S' .. T - 1 is set to 0; h_dense rows there stay unwritten;
 *   retired_at [N] int32 receives s0 + S', the number of samples evaluated, if the ray is retired or this is the last slab.
 * live_next [n_live] int32 receives the rays that are neither retired nor through their last slab, in ascending order of their
 * position in `live` (so an ascending `live` gives an ascending live_next), *n_live_next (int32) their number.  live_next must not
 * overlap live.  workspace: l4dr_slab_update_workspace(n_live) bytes. */
int l4dr_slab_update(const float* sigma_c, const void* h_c, const float* z_vals, const int32_t* live, int64_t n_live, int64_t N,
                     int32_t T, int32_t s0, int32_t S, float sample_dist, float density_scale, int32_t active_sensor, float eps,
                     float* trans, float* sigma_dense, void* h_dense, int32_t* retired_at, int32_t* live_next,
                     int32_t* n_live_next, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_MARCH_H */
