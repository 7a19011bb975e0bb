"""numpy restatement of the occupancy grid of ``render(..., early_stop=eps, slab=S, occupancy=grid)`` (lidar4d_amd/occupancy.py, the
flags of ``l4d_sample_rays`` in include/lidar4d_hip.h, ``early_stop.run_skipping``): the bit packing, the slab flags, the march in
float64 and the bound the audit states.  No device, no torch, nothing of the package.

Flags, in float32 and in the kernel's order (every numpy operation on float32 arrays rounds once, as the kernel's does with
-ffp-contract=off): z_s = near + (far - near) * lin_s;  p = min(max(o + d * z, -bound), bound);  u = (p + bound) / (2 bound);
c = min(R - 1, max(0, (int)floor(u * R))) per axis;  cell i = (c_z R + c_y) R + c_x;  flag (r, k) = any set cell among the samples
k S .. min(T, (k + 1) S) - 1 of ray r.

The march, in float64: sample s has tau_s = delta_s * density_scale * sigma_s * (2 if active_sensor else 1), delta_s = z_{s+1} - z_s
and sample_dist for the last one, and the factor f_s = (1 - alpha_s) + 1e-15, alpha_s = 1 - exp(-tau_s).  Slab k of a ray is
evaluated iff the ray is alive and flagged in it; then trans *= the product of the slab's factors, and the ray is retired
(retired_at = the slab's end) if trans < eps.  A ray never retired has retired_at = T.  Sigma is kept at evaluated samples and is 0
everywhere else.  ``near`` marks the rays whose trans at a tested slab end lies within the factor (1 + band) of eps either way: there
float32 rounding may decide differently (tests/early_stop_ref.py: the tested float32 product is the exact one to within
2 T 2^-24 relative, far inside band = 1e-3).

The audit's bound.  Let D be a ray's sum of tau over its skipped samples in the FULL render (no retirement).  Skipping replaces the
skipped factors e^{-tau} by 1, so the transmittance in front of sample s grows by e^{D_s}, 0 <= D_s <= D.  Hence, up to the 1e-15 terms:
an evaluated sample's weight w' = w e^{D_s} lies in [w, w e^D]; the skipped samples' weights, sum alpha_s T_s <= 1 - prod over the
skipped (1 - alpha_s) = 1 - e^{-D}; so |d weights_sum| <= max(e^D - 1, 1 - e^{-D}) <= e^D - 1 + D and, z <= far,
|d depth| <= far (e^D - 1 + D).
"""
import numpy as np

import early_stop_ref as er

F32 = np.float32
D_MAX = 80.0  # check_audit: the largest skipped optical depth for which e^D is formed


def shell_mask(R, r0, r1, bound=1.0):
    """bool [R, R, R] indexed [z, y, x]: the cells whose centre lies between the radii r0 and r1 around the middle of the box"""
    c = ((np.arange(R) + 0.5) / R * 2.0 - 1.0) * bound
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt(xx ** 2 + yy ** 2 + zz ** 2)
    return (r >= r0) & (r <= r1)


def block_mask(R, B, seed, p=0.5):
    """bool [R, R, R]: blocks of B^3 cells, each set with probability p"""
    n = -(-R // B)
    coarse = np.random.default_rng(seed).random((n, n, n)) < p
    return np.repeat(np.repeat(np.repeat(coarse, B, 0), B, 1), B, 2)[:R, :R, :R]


# The masks of the march tests (tests/test_gpu_occupancy.py; pinned on the CPU oracle by tests/test_occupancy_cpu.py): on the mixed
# scene of the early-stop tests, 37 rays of 130 samples in slabs of 32, both skip slabs in front of the surfaces and evaluate fewer
# rows than the march without a grid at eps = 0 and at eps = 1e-3.  (A shell from 0.3 to 0.6 does not: at eps = 1e-3 it delays so
# many retirements that it evaluates MORE rows, 2112 against 2016 on the oracle.)
MARCH_MASKS = {"shell": lambda: shell_mask(33, 0.25, 0.55), "blocks": lambda: block_mask(12, 3, 1)}


def pack(mask):
    """bool [R, R, R] indexed [z, y, x] -> int32 [ceil(R^3 / 32)], cell i = (z R + y) R + x at bit i & 31 of word i >> 5."""
    flat = np.asarray(mask, bool).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, np.uint32)
    for i in np.flatnonzero(flat):
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words.view(np.int32)


def sample_cells(rays_o, rays_d, lin, near, far, bound, R, z_vals=None):
    """-> z [N, T] float32, cell [N, T] int64 (flat cell index of every sample).  z_vals: the samples' depths [N, T] where they are
    not the un-jittered ones (then lin, near and far are not read)."""
    o, d = np.asarray(rays_o, F32), np.asarray(rays_d, F32)
    bound = F32(bound)
    if z_vals is None:
        near, far = F32(near), F32(far)
        z = (near + (far - near) * np.asarray(lin, F32)).astype(F32)                  # [T]
        z = np.broadcast_to(z, (o.shape[0], z.shape[0])).copy()
    else:
        z = np.asarray(z_vals, F32)
    v = (o[:, None, :] + (d[:, None, :] * z[:, :, None]).astype(F32)).astype(F32)     # [N, T, 3]
    p = np.minimum(np.maximum(v, -bound), bound)
    u = ((p + bound).astype(F32) / (F32(2.0) * bound)).astype(F32)
    c = np.clip(np.floor((u * F32(R)).astype(F32)), 0, R - 1).astype(np.int64)
    cell = (c[..., 2] * R + c[..., 1]) * R + c[..., 0]
    return z, cell


def slab_flags(mask, rays_o, rays_d, lin, near, far, bound, slab, z_vals=None):
    """-> z [N, T] float32, flags [N, ceil(T / slab)] uint8"""
    mask = np.asarray(mask, bool)
    z, cell = sample_cells(rays_o, rays_d, lin, near, far, bound, mask.shape[0], z_vals)
    hit = mask.reshape(-1)[cell]
    T = z.shape[1]
    n_slabs = -(-T // slab)
    flags = np.zeros((z.shape[0], n_slabs), np.uint8)
    for k in range(n_slabs):
        flags[:, k] = hit[:, k * slab:min(T, (k + 1) * slab)].any(1)
    return z, flags


def optical_depth(sigma, z_vals, sample_dist, density_scale, active_sensor):
    """tau [N, T] float64"""
    z = np.asarray(z_vals, np.float64)
    delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], float(sample_dist))], axis=1)
    return delta * float(density_scale) * np.asarray(sigma, np.float64) * (2.0 if active_sensor else 1.0)


def march(sigma, z_vals, flags, slab, eps, sample_dist, density_scale, active_sensor, band=er.REL):
    """-> masked sigma [N, T] (sigma's dtype), retired_at [N] int32, near [N] bool, evaluated (int: rows of evaluated slabs)"""
    sigma = np.asarray(sigma)
    N, T = sigma.shape
    tau = optical_depth(sigma, z_vals, sample_dist, density_scale, active_sensor)
    f = (1.0 - (1.0 - np.exp(-tau))) + 1e-15
    masked = np.zeros_like(sigma)
    retired_at = np.full(N, T, np.int32)
    near = np.zeros(N, bool)
    evaluated = 0
    for r in range(N):
        trans = 1.0
        for k in range(-(-T // slab)):
            s0, s1 = k * slab, min(T, (k + 1) * slab)
            if not flags[r, k]:
                continue
            masked[r, s0:s1] = sigma[r, s0:s1]
            evaluated += s1 - s0
            trans *= float(np.prod(f[r, s0:s1]))
            if eps > 0 and eps / (1.0 + band) <= trans <= eps * (1.0 + band):
                near[r] = True
            if trans < eps:
                retired_at[r] = s1
                break
    return masked, retired_at, near, evaluated


def composite(sigma, z_vals, sample_dist, density_scale, active_sensor):
    """float64 weights [N, T], weights_sum [N], depth [N] of a dense sigma (composite_fwd's formula, without its 1e-15)."""
    tau = optical_depth(sigma, z_vals, sample_dist, density_scale, active_sensor)
    alpha = 1.0 - np.exp(-tau)
    trans = np.cumprod(np.concatenate([np.ones_like(alpha[:, :1]), 1.0 - alpha[:, :-1]], axis=1), axis=1)
    w = alpha * trans
    return w, w.sum(1), (w * np.asarray(z_vals, np.float64)).sum(1)


def skipped_samples(flags, slab, T):
    """bool [N, T]: the samples of the slabs whose flag is 0"""
    return ~np.repeat(np.asarray(flags, bool), slab, axis=1)[:, :T]


def check_audit(full, skipping, D, lost, skipped, far, slack=er.REL, t_abs=None, what=""):
    """The four inequalities, per ray.  full / skipping: dicts with weights [N, T], weights_sum [N], depth [N] of the full render and
    of the render that skips; D, lost [N]: the audit's; skipped [N, T] bool.  slack: relative room for float32 rounding (the
    early-stop bound's own, 1e-3) on top of one float32 unit of a weight (alpha = 1 - exp(.) is formed to 2^-24 absolute).  t_abs:
    the absolute error of the full render's transmittance (default: float32's, below; 0 for float64 renders)."""
    w, ws = np.asarray(full["weights"], np.float64), np.asarray(skipping["weights"], np.float64)
    D, lost = np.asarray(D, np.float64), np.asarray(lost, np.float64)
    unit = 2.0 ** -23
    # What float32 does to "w' <= w e^D".  A factor (1 - alpha) + 1e-15 with alpha = 1 - exp(-tau) is formed to about 2^-24 ABSOLUTE
    # -- for tau > 17 it is 1e-15 whatever tau is -- and every factor is at most 1, so the full render's transmittance in front of
    # a sample, and with it the weight w, is off by up to t_abs = 2 (T + 1) 2^-24 absolute.  Skipping divides by the skipped
    # factors, which multiplies that error by e^D like w itself: w' <= (w + t_abs) e^D.  The test says something for
    # e^D t_abs < 1, D below 11 at T = 130; beyond, a weight of 1 is inside the bound.  (e^D is formed for D <= D_MAX: above it
    # every bound here exceeds 1e29, more than any weight or sum of weights.)  Summed over a ray's T samples the same term enters the
    # bounds on weights_sum and depth.  A ray with D = 0 is not left to these: its weights are the full render's bits (the GPU test).
    t_abs = 2.0 * (w.shape[1] + 1) * 2.0 ** -24 if t_abs is None else t_abs
    capped = np.minimum(D, D_MAX)
    grow = np.exp(capped)[:, None]
    ev = ~skipped
    assert (ws[skipped] == 0).all(), (what, "a skipped sample has weight")
    assert (ws[ev] >= (w * (1.0 - slack) - unit)[ev]).all(), (what, "an evaluated weight fell")
    upper = ev & (D <= D_MAX)[:, None]
    assert (ws[upper] <= ((w + t_abs) * grow * (1.0 + slack) + unit)[upper]).all(), (what, "an evaluated weight grew by more than e^D")
    assert (lost <= (1.0 - np.exp(-D)) * (1.0 + slack) + unit * w.shape[1]).all(), (what, "lost weight above 1 - e^-D")
    bound = (np.exp(capped) - 1.0 + capped) * (1.0 + slack) + w.shape[1] * (t_abs * np.exp(capped) + unit)
    d = np.abs(np.asarray(full["weights_sum"], np.float64) - np.asarray(skipping["weights_sum"], np.float64))
    assert (d <= bound).all(), (what, "weights_sum", d.max())
    d = np.abs(np.asarray(full["depth"], np.float64) - np.asarray(skipping["depth"], np.float64))
    assert (d <= far * bound).all(), (what, "depth", d.max())
