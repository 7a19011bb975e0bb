"""numpy restatement of the early-termination rule of ``render(..., early_stop=eps, slab=S)`` (include/lidar4d_march.h,
lidar4d_amd/early_stop.py) and the bound its result keeps.  No device, no torch.

The rule, in float32 and in slab_update_kernel's order (csrc/raymarch.hip).  Sample k of a ray has the factor
``f_k = (1 - alpha_k) + 1e-15`` with ``alpha_k = 1 - exp(-(2 if active_sensor else 1) * delta_k * density_scale * sigma_k)``,
``delta_k = z_{k+1} - z_k`` and ``sample_dist`` for the last sample: composite_fwd's alpha (renderer.py:98-104 of the reference).
A slab is the samples ``s0 .. s0 + S' - 1``, ``S' = min(S, T - s0)``.  Lane ``l`` of 64 multiplies the factors of samples
``s0 + l, s0 + l + 64, ...`` in that order starting from the first (a lane without a sample holds 1), the lane products are
combined by the tree ``v[l] = v[l] * v[l + o]`` for ``o = 32, 16, ... 1``, and ``trans = trans * v[0]``.  The ray is retired after the slab
if ``trans < eps`` (false for a NaN); a retired ray's remaining samples count as sigma = 0.

The bound.  Let T_s be the exact product of the factors of the samples in front of s (the transmittance composite_fwd's weights are
built from, ``w_k = alpha_k T_k``), and let a ray be retired after the slab that ends in front of sample s.

* The tested value T^ is a product of at most T float32 factors taken in some order, each multiplication rounding once:
  ``T^ = T_s (1 + theta)``, ``|theta| <= (1 + 2^-24)^T - 1 <= 2 T 2^-24``, which is 9.2e-5 < 1e-4 for T = 768 (the plain render's
  own running product has an error of the same size).  So ``T^ < eps`` gives ``T_s < eps (1 + 1e-3) = eps'`` with room to spare.
* ``1 - alpha_k = f_k - 1e-15 <= f_k``, so the weights telescope: ``sum_{k >= s} w_k = sum (1 - (1 - alpha_k)) T_k <= T_s - T_end <= T_s``
  up to the 1e-15 terms, T * 1e-15.  The culled weights of a ray sum to less than eps'.
* Hence ``|d weights_sum| <= eps'``; z <= far_lidar gives ``|d depth| <= eps' * far_lidar``; every culled sample's weight is below
  eps', and attribute values lie in [0, 1] (sigmoid), so ``|d image| <= eps'``.
* A sample in front of s has the same sigma, the same alpha and the same prefix product as in the plain render: weights, mask
  entries and attribute values there are the plain render's bits.
* For ``eps <= 5e-5``, eps' < 1e-4: no culled sample has ``w > 1e-4``, the mask list and therefore image_lidar (a sum over the mask
  list's samples; all others contribute attr = 0) are the plain render's.
* ``eps = 0``: ``trans < 0`` never holds, no ray is retired, every output is the plain render's.
"""
import numpy as np

F32 = np.float32
REL = 1e-3  # eps' = eps * (1 + REL)


def eps_prime(eps):
    return eps * (1.0 + REL)


def factors(sigma, z_vals, sample_dist, density_scale, active_sensor, exp=np.exp):
    """f [N, T] float32, every operation rounded to float32 in render.hip's order.  exp: the float32 exponential to use (a test
    that compares bits hands in the device's)."""
    sigma, z = np.asarray(sigma, F32), np.asarray(z_vals, F32)
    delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], F32(sample_dist))], axis=1).astype(F32)
    with np.errstate(all="ignore"):
        e = ((F32(-2.0) * delta if active_sensor else -delta) * F32(density_scale)).astype(F32) * sigma
        alpha = F32(1.0) - np.asarray(exp(e.astype(F32)), F32)
        return ((F32(1.0) - alpha).astype(F32) + F32(1e-15)).astype(F32)


def slab_product(f):
    """The product of one ray's factors of one slab (1-D float32, any length >= 1) in the kernel's order."""
    f = np.asarray(f, F32)
    v = np.ones(64, F32)
    with np.errstate(all="ignore"):
        for l in range(min(64, f.shape[0])):
            p = f[l]
            for k in range(l + 64, f.shape[0], 64):
                p = F32(p * f[k])
            v[l] = p
        for o in (32, 16, 8, 4, 2, 1):
            v[:o] = v[:o] * v[o:2 * o]
    return v[0]


def march(f, S, eps):
    """f [N, T] float32 factors -> (trans [N] float32 at each ray's end, retired_at [N] int32 = samples evaluated,
    live_lists = the ascending live list in front of every slab that runs)."""
    f = np.asarray(f, F32)
    N, T = f.shape
    trans = np.ones(N, F32)
    retired_at = np.zeros(N, np.int32)
    live, lists, s0 = list(range(N)), [], 0
    eps = F32(eps)
    while s0 < T and live:
        lists.append(list(live))
        Sp = min(S, T - s0)
        nxt = []
        for r in live:
            with np.errstate(all="ignore"):
                trans[r] = F32(trans[r] * slab_product(f[r, s0:s0 + Sp]))
            retired = bool(trans[r] < eps)
            if retired or s0 + Sp >= T:
                retired_at[r] = s0 + Sp
            else:
                nxt.append(r)
        live, s0 = nxt, s0 + Sp
    return trans, retired_at, lists


def transmittance_from_weights(weights):
    """T [N, T + 1] float64 from a full render's weights: T_0 = 1, T_{s+1} = T_s - w_s (w_s = alpha_s T_s)."""
    w = np.asarray(weights, np.float64)
    return np.concatenate([np.ones_like(w[:, :1]), 1.0 - np.cumsum(w, axis=1)], axis=1)


def predict_retirement(weights, S, eps, band):
    """From a full render's weights: retired_at [N] (T for a ray that is never retired) and ``near`` [N] bool: the ray's transmittance
    at some slab end up to its retirement lies within the factor (1 + band) of eps either way, so that rounding may decide."""
    trans = transmittance_from_weights(weights)
    N, T = np.asarray(weights).shape
    retired_at = np.full(N, T, np.int32)
    near = np.zeros(N, bool)
    for r in range(N):
        for end in list(range(S, T, S)) + [T]:
            t = trans[r, end]
            if eps > 0 and eps / (1.0 + band) <= t <= eps * (1.0 + band):
                near[r] = True
            if t < eps or end == T:
                retired_at[r] = end
                break
    return retired_at, near


def cull(values, retired_at):
    """values [N, T, ...] with zeros behind each ray's retirement point."""
    out = np.array(values, copy=True)
    for r, s in enumerate(retired_at):
        out[r, int(s):] = 0
    return out


def check_bound(full, culled, eps, far, what=""):
    """full / culled: dicts with weights [N, T], weights_sum [N], depth [N] and optionally image [N, C].  Asserts the bound above."""
    e = eps_prime(eps)
    dw = np.asarray(full["weights"], np.float64) - np.asarray(culled["weights"], np.float64)
    assert dw.min() >= 0.0 and dw.max() <= e, (what, "culled weight", dw.min(), dw.max(), e)
    d = np.abs(np.asarray(full["weights_sum"], np.float64) - np.asarray(culled["weights_sum"], np.float64)).max()
    assert d <= e, (what, "weights_sum", d, e)
    d = np.abs(np.asarray(full["depth"], np.float64) - np.asarray(culled["depth"], np.float64)).max()
    assert d <= e * far, (what, "depth", d, e * far)
    if "image" in full:
        d = np.abs(np.asarray(full["image"], np.float64) - np.asarray(culled["image"], np.float64)).max()
        assert d <= (0.0 if eps <= 5e-5 else e), (what, "image", d, e)
