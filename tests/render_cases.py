"""Inputs and references for the edge-shape tests of ray sampling and compositing (tests/test_render_cpu.py,
tests/test_gpu_render_edges.py): sample_rays_kernel, composite_fwd_kernel with its mask and work list, composite_image_kernel and
composite_bwd_kernel of csrc/render.hip, and the dense sample_rays_xt_kernel of csrc/fused.hip.  numpy only: importable without
a device, and nothing here is computed by HIP code.

Three kinds of reference, named as in tests/glue_cases.py.

E, exact emulation (sampling).  The library is compiled without fma contraction and with IEEE division, so sample_depth,
ray_point and unit_coord of csrc/render_dev.h are re-evaluated in numpy float32 in the order they are written.  Bit-equal.

S, saturated lattice (compositing structure).  z = (j + 1) / 16384, sample_dist = 2^-14, density_scale a power of two, sigma 0
except "opaque" samples of 3e7: alpha is exactly 0 (expf(-0) = 1) or exactly 1 (expf(-1831) = 0), every factor of the
transmittance is 1 or 1e-15f, and nothing depends on the order of a product or a sum.  The upstream gradients lie on a lattice
(``assert_lattice``), so the adjoint's g_i is exact too.  The expected outputs are CLOSED FORMS written down here (one-hot weights,
(g_i - g_p) c in front of the opaque sample, fl32(g_i 1e-15f) c behind it); tests/test_render_cpu.py shows that a float32
restatement of the kernels' scans and carries gives them exactly, and that a carry moved by one sample or a dropped segment
carry in that restatement does not.  Equal values (+0 == -0 where a product with (1 - alpha) = 0 leaves the sign free).

N, numerics against float64.  ``composite_ref64`` / ``composite_bwd_ref64`` from the float32 inputs: alpha = -expm1(-x),
x = kappa delta density_scale sigma, factor exp(-x) + 1e-15, cumulative product; the adjoint is the closed form in the comment
above composite_bwd_kernel.  Inputs are well conditioned: sigma = u^4 3 T keeps a sample's optical depth independent of T
(alpha up to about 0.96; T = 1 and 2 have the long intervals, where 1 - alpha goes down to 3e-6, still 50 fp32 ulps of 1).  |got - ref| <= atol + rtol |ref| with the tolerances of
tests/test_gpu_ops.py::test_composite_bwd (TOL below).  Every tolerance is first shown on the CPU to hold, with a factor four to
spare, for ``composite_fwd_f32`` / ``composite_bwd_f32``: numpy float32 restatements in the kernels' order (Hillis-Steele scans
over 64 lanes, chunk carry, segment carry, suffix carry, butterfly reductions).  The factor covers the device's expf (documented
at 1 ulp) differing from numpy's, and the reductions.  d_sigma's absolute term is DSIGMA_K max|ref d_sigma| over the case, and
DSIGMA_K is four times the restatement's largest excess -- it is never taken from the kernel.

Largest excess over the rtol term, max(|x - ref| - rtol |ref|), over the numeric cases (NUMERIC_CASES); negative = inside the
rtol term alone.  CPU: the float32 restatement, printed by tests/test_render_cpu.py.  MI355X: the kernels, printed by
tests/test_gpu_render_edges.py.
                                   CPU restatement      MI355X           allowed (atol)
    weights                        +2.92e-8             +3.35e-8         3e-7
    weights_sum, depth, image      +2.67e-8             +2.67e-8         3e-7
    d_attr                         +2.84e-8             +2.95e-8         3e-7
    d_sigma / max|ref d_sigma|     +5.48e-7             +5.48e-7         DSIGMA_K = 2.2e-6
    mask away from the reference   0 samples            0 samples        only borderline samples (at most 1 of a case's
                                                                         99 .. 232 kept samples is borderline: below 1 %)
(d_sigma's excess is the same on both to three digits: one sample of the T = 1023 passive case sets it.)
"""
import numpy as np

from glue_cases import F32, F64, assert_lattice, rng_of, same_bits, to_f32_exact  # noqa: F401  (same_bits: for the tests)

T_EDGES = (1, 2, 63, 64, 65, 128, 1023, 1024, 1025, 2049, 8192)
N_EDGES = (1, 3, 4, 5, 15, 16, 17, 33)
CHUNK, SEGMENT = 64, 1024        # csrc/render.hip: samples per scan, samples per segment (MAXC = 16 chunks)
FWD_RAYS, BWD_RAYS = 16, 4       # rays per workgroup of composite_fwd_kernel / composite_bwd_kernel and composite_image_kernel
T_MAX, C_MAX = 8192, 4           # what l4d_composite_bwd accepts
EPS_T = F32(1e-15)               # the 1e-15f of (1 - alpha) + 1e-15f
MASK_THRESHOLD = F32(1e-4)


def lin_of(T):
    """[T] fp32 in [0, 1], [0] for T = 1.  An input like any other: the device tests of sampling use torch.linspace's bits."""
    return np.linspace(0.0, 1.0, T).astype(F32)


# =================================================================================================================================
# 1. sampling, class E
# =================================================================================================================================
SAMPLE_SHAPES = [(1, 1), (1, 255), (3, 85), (1, 256), (1, 257), (5, 768), (33, 1025)]  # around the 256-thread workgroup
SAMPLE_BOUNDS = (1.0, 2.0, 1.3)   # 2 bound a power of two (the division is exact) and not
SAMPLE_NEAR, SAMPLE_FAR = 0.0105, 0.851
SAMPLE_T = F32(0.3701171)
NOISE_MAX = np.nextafter(F32(1.0), F32(0.0))


def sample_ref(rays_o, rays_d, lin, noise, near, far, bound, t=SAMPLE_T):
    """E.  -> z_vals [N,T], xyz [N*T,3], xt [N*T,4], beyond [N,T,3] int8 (-1 / 0 / +1: the unclamped point lies beyond that face)."""
    ro, rd, lin = np.asarray(rays_o), np.asarray(rays_d), np.asarray(lin)
    assert ro.dtype == rd.dtype == lin.dtype == F32
    near, far, bound = F32(near), F32(far), F32(bound)
    N, T = ro.shape[0], lin.shape[0]
    z = np.broadcast_to(near + (far - near) * lin, (N, T)).copy()           # sample_depth
    if noise is not None:
        assert noise.dtype == F32 and noise.shape == (N, T)
        sample_dist = (far - near) / F32(T)
        z = z + (noise - F32(0.5)) * sample_dist
    v = ro[:, None, :] + rd[:, None, :] * z[:, :, None]                     # ray_point: product rounded, then sum rounded
    xyz = np.minimum(np.maximum(v, -bound), bound)
    xt = np.empty((N, T, 4), F32)
    xt[:, :, :3] = (xyz + bound) / (F32(2.0) * bound)                       # unit_coord
    xt[:, :, 3] = F32(t)
    assert z.dtype == xyz.dtype == F32
    beyond = (v > bound).astype(np.int8) - (v < -bound).astype(np.int8)
    return z, xyz.reshape(N * T, 3), xt.reshape(N * T, 4), beyond


def sample_case(N, T, bi, with_noise):
    """Rays that leave the box: axis k of ray r heads for the face of sign (-1)^(r + bi + r k), from an origin 5 .. 40 % of the
    bound inside it with a direction component of 60 .. 100 % of the bound (the far end, z = 0.851, is clamped; the near end is
    not).  T = 1 has one sample per ray, at z in [-0.41, 0.43] with noise: its origins lie half a bound OUTSIDE the face, so the
    sample is clamped on three faces.  noise holds 0 and the largest fp32 below 1."""
    bound = SAMPLE_BOUNDS[bi]
    r = rng_of(31, N, T, bi)
    ray, k = np.arange(N)[:, None], np.arange(3)[None, :]
    sign = np.where((ray + bi + ray * k) % 2 == 0, 1.0, -1.0)
    inside = r.uniform(0.05, 0.4, size=(N, 3)) if T > 1 else np.full((N, 3), -0.5)
    rays_o = (sign * bound * (1.0 - inside)).astype(F32)
    rays_d = (sign * bound * r.uniform(0.6, 1.0, size=(N, 3))).astype(F32)
    noise = None
    if with_noise:
        noise = r.uniform(0.0, 1.0, size=(N, T)).astype(F32)
        noise[noise >= 1.0] = NOISE_MAX
        if N * T > 1:
            noise.reshape(-1)[0], noise.reshape(-1)[-1] = F32(0.0), NOISE_MAX
        else:
            noise[0, 0] = (F32(0.0), NOISE_MAX, F32(0.5))[bi]
    return dict(rays_o=rays_o, rays_d=rays_d, noise=noise, near=SAMPLE_NEAR, far=SAMPLE_FAR, bound=bound, N=N, T=T)


def sample_cases(N, T, with_noise):
    """The three bounds of one shape.  One ray reaches three faces, so the three bounds take the six between them (the sign
    pattern turns with the bound's index); ASSERTED here with ``lin_of``: each of the six faces clamps some sample of the shape,
    clamped coordinates are exactly 0 / 1 in xt, and for T > 1 every bound also has samples inside the box."""
    cases = [sample_case(N, T, bi, with_noise) for bi in range(len(SAMPLE_BOUNDS))]
    faces = set()
    for c in cases:
        _, _, xt, beyond = sample_ref(c["rays_o"], c["rays_d"], lin_of(T), c["noise"], c["near"], c["far"], c["bound"])
        b = beyond.reshape(-1, 3)
        faces |= {(k, s) for k in range(3) for s in (-1, 1) if (b[:, k] == s).any()}
        assert (xt[:, :3][b == 1] == 1.0).all() and (xt[:, :3][b == -1] == 0.0).all()
        assert T == 1 or (b == 0).any(), "no sample inside the box"
        if with_noise:
            assert (c["noise"] == 0).any() or N * T == 1
            assert (c["noise"] == NOISE_MAX).any() or N * T == 1
            assert (c["noise"] < 1).all() and (c["noise"] >= 0).all()
    assert len(faces) == 6, f"N={N} T={T}: only the faces {sorted(faces)} clamp a sample"
    if with_noise and N * T == 1:
        assert {float(c["noise"][0, 0]) for c in cases} >= {0.0, float(NOISE_MAX)}
    return cases


# =================================================================================================================================
# 2. compositing structure, class S
# =================================================================================================================================
Z_UNIT = 2.0 ** -14
STRUCT_SIGMA = F32(3e7)
STRUCT_P = (0, 1, 62, 63, 64, 65, 127, 128, 1022, 1023, 1024, 1025, 2047, 2048, -2, -1)  # chunk and segment edges, both ends
STRUCT_SHAPES = [(33, T) for T in T_EDGES] + [(N, T) for T in (65, 1025) for N in N_EDGES if N != 33]
STRUCT_MULTI = {  # T -> opaque samples (p < q [< s]) per ray, in different chunks and different segments
    130: [(3, 64), (63, 64, 128), (0, 65, 129), (127, 128)],
    1025: [(3, 1024), (1023, 1024), (0, 63, 1024), (62, 1023, 1024), (64, 1000)],
    2049: [(1023, 1024, 2048), (0, 1024, 2048), (5, 2047, 2048), (1024, 2048)],
    8192: [(0, 4095, 8191), (3, 1024), (1023, 1024, 2048), (1024, 7168, 8191), (7167, 7168)],
}
GUARD_N = (1, 15, 17)
GUARD_T = (65, 1025)


def struct_positions(N, T):
    """The opaque sample of every ray: STRUCT_P inside [0, T), in that order without repeats, dealt to the rays in turn."""
    cand = []
    for p in STRUCT_P:
        p = p + T if p < 0 else p
        if 0 <= p < T and p not in cand:
            cand.append(p)
    return np.array([cand[r % len(cand)] for r in range(N)], np.int64)


def struct_inputs(N, T, active, positions=None):
    """-> dict(sigma, z [N,T] fp32, sample_dist, density_scale, active, opaque: list of tuples per ray)."""
    if positions is None:
        positions = [(int(p),) for p in struct_positions(N, T)]
    assert len(positions) == N and all(0 <= p < T for ps in positions for p in ps)
    assert all(len(ps) <= 3 and list(ps) == sorted(set(ps)) for ps in positions), "a fourth factor of 1e-15f is denormal"
    z = np.broadcast_to(to_f32_exact((np.arange(T) + 1.0) * Z_UNIT), (N, T)).copy()
    sigma = np.zeros((N, T), F32)
    for r, ps in enumerate(positions):
        sigma[r, list(ps)] = STRUCT_SIGMA
    c = dict(sigma=sigma, z=z, sample_dist=Z_UNIT, density_scale=2.0 if active else 1.0, active=bool(active), opaque=positions,
             N=N, T=T)
    # the saturation itself, in float32 as alpha_of writes it
    kappa = 2.0 if active else 1.0
    with np.errstate(under="ignore"):
        e = np.exp((F32(-kappa * Z_UNIT) * F32(c["density_scale"])) * STRUCT_SIGMA)
    assert e.dtype == F32 and e == 0.0 and float(kappa * Z_UNIT * c["density_scale"] * 3e7) > 1800.0
    assert F32(1.0) + EPS_T == F32(1.0)
    return c


def struct_fwd_ref(c):
    """-> weights [N,T], weights_sum [N], depth [N] fp32, mask [N,T] uint8, idx (sorted) int32.  Weights 1, 1e-15f,
    fl32(1e-15f 1e-15f) on the opaque samples in order; their sum is 1 and the depth z_p in any order (the later terms are below
    2^-49 and 2^-50 z, half an ulp of 1 and of z_p >= 2^-14 are 2^-25 and 2^-38); only the first is above 1e-4."""
    N, T = c["N"], c["T"]
    w = np.zeros((N, T), F32)
    mask = np.zeros((N, T), np.uint8)
    vals = (F32(1.0), EPS_T, EPS_T * EPS_T)
    assert vals[2].dtype == F32 and vals[2] > 1e-37
    for r, ps in enumerate(c["opaque"]):
        for v, p in zip(vals, ps):
            w[r, p] = v
        mask[r, ps[0]] = 1
    first = np.array([ps[0] for ps in c["opaque"]], np.int64)
    depth = c["z"][np.arange(N), first].copy()
    idx = (np.arange(N, dtype=np.int64) * T + first).astype(np.int32)
    return dict(weights=w, weights_sum=np.ones(N, F32), depth=depth, mask=mask, idx=idx, count=N)


def struct_attr(N, T, C):
    """[N*T, C] fp32 multiples of 1/8 in [-1, 1]."""
    r, j, ch = np.arange(N)[:, None, None], np.arange(T)[None, :, None], np.arange(C)[None, None, :]
    return to_f32_exact(((r * 7 + j * 3 + ch * 5) % 17 - 8) / 8.0).reshape(N * T, C)


def struct_image_ref(c, attr, C):
    """image[r] = attr[r, p_r]: one weight is 1, the others are 0 (rays with one opaque sample)."""
    assert all(len(ps) == 1 for ps in c["opaque"])
    p = np.array([ps[0] for ps in c["opaque"]])
    return attr.reshape(c["N"], c["T"], C)[np.arange(c["N"]), p].copy()


def struct_grads(N, T, C):
    """Upstream gradients on their lattices: d_depth, d_image integers in [-2, 2], d_wsum multiples of 1/4 in [-2, 2], d_weights
    multiples of 1/16 in [-4, 4]; every one of them non-zero somewhere (where the shape has room)."""
    r = rng_of(37, N, T, C)
    g = dict(d_depth=r.randint(-2, 3, size=N).astype(F32), d_wsum=(r.randint(-8, 9, size=N) / 4.0).astype(F32),
             d_image=r.randint(-2, 3, size=(N, max(C, 1))).astype(F32)[:, :C].copy(),
             d_weights=(r.randint(-64, 65, size=(N, T)) / 16.0).astype(F32))
    g["d_depth"][0], g["d_wsum"][0] = F32(-2.0), F32(0.75)
    if C:
        g["d_image"][0] = F32(1.0)
    return g


def struct_g(c, attr, C, grads):
    """g_i = d_depth z_i + d_wsum + d_weights_i + sum_c d_image_c attr_ic with absent gradients left out: float64, asserted equal
    to the float32 evaluation in the kernel's order and to lie on the lattice of 2^-14.  grads: dict, None = null pointer."""
    N, T = c["N"], c["T"]
    z32 = c["z"]
    g64 = np.zeros((N, T))
    g32 = np.zeros((N, T), F32)
    terms = []
    if grads.get("d_depth") is not None:
        terms.append(grads["d_depth"].astype(F64)[:, None] * z32.astype(F64))
        g32 = grads["d_depth"][:, None] * z32 + g32
    if grads.get("d_wsum") is not None:
        terms.append(np.broadcast_to(grads["d_wsum"].astype(F64)[:, None], (N, T)))
        g32 = g32 + grads["d_wsum"][:, None]
    if grads.get("d_weights") is not None:
        terms.append(grads["d_weights"].astype(F64))
        g32 = g32 + grads["d_weights"]
    if attr is not None and C and grads.get("d_image") is not None:
        a = attr.reshape(N, T, C)
        for ch in range(C):
            terms.append(grads["d_image"].astype(F64)[:, None, ch] * a[:, :, ch].astype(F64))
            g32 = g32 + grads["d_image"][:, None, ch] * a[:, :, ch]
    if terms:
        st = np.stack(terms)
        assert_lattice(st, Z_UNIT, axis=0, what="g")
        g64 = st.sum(0)
    assert g32.dtype == F32 and (g32.astype(F64) == g64).all(), "g is not exact in fp32"
    return g64


def struct_bwd_ref(c, attr, C, grads, want_d_attr=True):
    """Rays with one opaque sample p.  -> d_sigma [N,T] fp32, d_attr [N*T,C] fp32 or None.  With c = kappa 2^-14 density_scale (a
    power of two): (g_i - g_p) c in front of p (transmittance 1, the suffix is g_p w_p = g_p), 0 at p ((1 - alpha) = 0),
    fl32(g_i 1e-15f) c behind it (transmittance 1e-15f, empty suffix).  d_attr = weights (x) d_image."""
    N, T = c["N"], c["T"]
    assert all(len(ps) == 1 for ps in c["opaque"])
    p = np.array([ps[0] for ps in c["opaque"]])
    g = struct_g(c, attr, C, grads)
    cc = (2.0 if c["active"] else 1.0) * Z_UNIT * c["density_scale"]
    assert np.log2(cc) == np.rint(np.log2(cc))
    j = np.arange(T)[None, :]
    gp = g[np.arange(N), p][:, None]
    front = to_f32_exact((g - gp) * cc, "d_sigma in front of the opaque sample")
    behind = (to_f32_exact(g) * EPS_T) * F32(cc)
    assert behind.dtype == F32 and (np.abs(behind[behind != 0]) > 1e-30).all(), "a denormal product"
    d_sigma = np.where(j < p[:, None], front, np.where(j == p[:, None], F32(0.0), behind)).astype(F32)
    d_attr = None
    if want_d_attr and C:
        di = grads["d_image"] if grads.get("d_image") is not None else np.zeros((N, C), F32)
        d_attr = np.zeros((N, T, C), F32)
        d_attr[np.arange(N), p] = di
        d_attr = d_attr.reshape(N * T, C)
    return d_sigma, d_attr


def assert_values(got, want, what):
    """Equal values element by element (+0 == -0), no NaN on either side."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(~(got == want).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} differ, first at {bad[:6]}: got {got.reshape(-1)[bad[:6]]}, "
                           f"want {want.reshape(-1)[bad[:6]]}")


def struct_check_fwd(c, got):
    """got: dict(weights, weights_sum, depth[, mask][, idx, count]) of numpy arrays, idx as the kernel wrote it."""
    ref = struct_fwd_ref(c)
    for k in ("weights", "weights_sum", "depth"):
        assert_values(got[k], ref[k], f"{k} N={c['N']} T={c['T']}")
    if got.get("mask") is not None:
        assert_values(got["mask"], ref["mask"], "mask")
    if got.get("idx") is not None:
        assert int(got["count"]) == ref["count"], (int(got["count"]), ref["count"])
        assert_values(np.sort(got["idx"][:ref["count"]]), ref["idx"], "work list")


def struct_check_bwd(c, attr, C, grads, d_sigma, d_attr, want_d_attr=True):
    ref_s, ref_a = struct_bwd_ref(c, attr, C, grads, want_d_attr)
    assert_values(d_sigma, ref_s, f"d_sigma N={c['N']} T={c['T']} C={C}")
    if ref_a is not None:
        assert_values(d_attr, ref_a, f"d_attr N={c['N']} T={c['T']} C={C}")


# =================================================================================================================================
# 3. compositing numerics, class N
# =================================================================================================================================
NUMERIC_N = 19
NUMERIC_DENSITY_SCALE = 1.3
NUMERIC_CASES = ([(NUMERIC_N, T, a, 2) for T in T_EDGES for a in (False, True)] +
                 [(NUMERIC_N, T, a, C) for T in (65, 1025) for a in (False, True) for C in (1, 3, 4)])
TOL = {  # (rtol, atol): tests/test_gpu_ops.py::test_composite_bwd and the golden test
    "weights": (3e-5, 3e-7), "weights_sum": (1e-4, 3e-7), "depth": (1e-4, 3e-7), "image": (1e-4, 3e-7), "d_attr": (1e-4, 3e-7),
}
DSIGMA_RTOL = 2e-3
# atol(d_sigma) = DSIGMA_K max|ref d_sigma| of the case.  Four times the largest excess over the rtol term of the float32
# restatement against float64, relative to max|ref d_sigma|, over NUMERIC_CASES: measured 5.48e-7 (T = 1023, passive) by
# tests/test_render_cpu.py::test_restatement_meets_every_tolerance_with_a_factor_four, which asserts 4 x measured <= DSIGMA_K.
DSIGMA_K = 2.2e-6
BORDERLINE_CAP = 0.01


def numeric_case(N, T, active, C):
    """z from the sampling restatement (near 0.0105, far 0.851, noise), sigma = u^4 3 T, gradients uniform in [-1, 1], attr in
    [0, 1].  Rows depend on (T, ray) only, so ray r of the N = 33 batch is ray r of any other."""
    def u(key, lo, hi, cols=()):
        return np.stack([rng_of(41, key, T, r).uniform(lo, hi, size=(T,) + cols) for r in range(N)]).astype(F32)
    noise = np.minimum(u(1, 0.0, 1.0), NOISE_MAX)
    zero = np.zeros((N, 3), F32)
    z = sample_ref(zero, zero, lin_of(T), noise, 0.0105, 0.851, 1.0)[0]
    sample_dist = float((F32(0.851) - F32(0.0105)) / F32(T))
    sigma = (u(2, 0.0, 1.0).astype(F64) ** 4 * (3.0 * T)).astype(F32)
    return dict(N=N, T=T, active=bool(active), C=C, z=z, sigma=sigma, sample_dist=sample_dist, density_scale=NUMERIC_DENSITY_SCALE,
                attr=u(3, 0.0, 1.0, (C,)).reshape(N * T, C), d_depth=u(4, -1.0, 1.0)[:, 0].copy(), d_wsum=u(5, -1.0, 1.0)[:, 0].copy(),
                d_image=u(6, -1.0, 1.0, (C,))[:, 0].copy(), d_weights=u(7, -1.0, 1.0))


def take_rays(c, rays):
    """The case restricted to ``rays`` (a list)."""
    N, T, C = c["N"], c["T"], c["C"]
    out = dict(c, N=len(rays))
    for k in ("z", "sigma", "d_depth", "d_wsum", "d_image", "d_weights"):
        out[k] = np.ascontiguousarray(c[k][rays])
    out["attr"] = np.ascontiguousarray(c["attr"].reshape(N, T, C)[rays]).reshape(len(rays) * T, C)
    return out


def _x64(sigma, z, sample_dist, density_scale, active):
    s, zz = np.asarray(sigma).astype(F64), np.asarray(z).astype(F64)
    delta = np.concatenate([zz[:, 1:] - zz[:, :-1], np.full_like(zz[:, :1], float(F32(sample_dist)))], axis=1)
    kd = (2.0 if active else 1.0) * delta * float(F32(density_scale))
    return kd * s, kd


def composite_ref64(sigma, z, sample_dist, density_scale, active, attr=None, C=0):
    """Float64 forward from the float32 inputs.  -> dict(weights, weights_sum, depth[, image], trans, fac, dalpha)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x, kd = _x64(sigma, z, sample_dist, density_scale, active)
        alpha = -np.expm1(-x)
        fac = np.exp(-x) + float(EPS_T)
        trans = np.concatenate([np.ones_like(fac[:, :1]), np.cumprod(fac, axis=1)[:, :-1]], axis=1)
        w = alpha * trans
        out = dict(weights=w, weights_sum=w.sum(1), depth=(w * np.asarray(z).astype(F64)).sum(1), trans=trans, fac=fac,
                   dalpha=kd * np.exp(-x))  # d alpha / d sigma = kappa delta density_scale (1 - alpha)
    if attr is not None and C:
        out["image"] = (w[:, :, None] * np.asarray(attr).astype(F64).reshape(w.shape + (C,))).sum(1)
    return out


def composite_bwd_ref64(c, fwd=None):
    """Float64 adjoint, the closed form above composite_bwd_kernel: dL/dalpha_i = g_i T_i - (sum_{k>i} g_k w_k) / (1 - alpha_i + eps).
    -> d_sigma [N,T], d_attr [N*T,C]."""
    N, T, C = c["N"], c["T"], c["C"]
    f = fwd or composite_ref64(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], c["active"])
    attr = c["attr"].astype(F64).reshape(N, T, C)
    di = c["d_image"].astype(F64)
    g = (c["d_depth"].astype(F64)[:, None] * c["z"].astype(F64) + c["d_wsum"].astype(F64)[:, None] + c["d_weights"].astype(F64) +
         (attr * di[:, None, :]).sum(2))
    q = g * f["weights"]
    suffix = np.cumsum(q[:, ::-1], axis=1)[:, ::-1] - q
    d_sigma = (g * f["trans"] - suffix / f["fac"]) * f["dalpha"]
    return d_sigma, (f["weights"][:, :, None] * di[:, None, :]).reshape(N * T, C)


def excess(got, ref, rtol):
    """max(|got - ref| - rtol |ref|): what an absolute term has to cover."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float(np.max(np.abs(got - ref) - rtol * np.abs(ref)))


def assert_close(got, ref, rtol, atol, what):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) - (atol + rtol * np.abs(ref))
    bad = np.flatnonzero(~(err.reshape(-1) <= 0))
    assert bad.size == 0, (f"{what}: {bad.size} of {ref.size} outside rtol {rtol} atol {atol}, worst at {int(np.nanargmax(err))}: got "
                           f"{got.reshape(-1)[bad[:4]]}, want {ref.reshape(-1)[bad[:4]]}")


def borderline(w_ref):
    """Samples whose float64 weight lies within the weights tolerance of the mask threshold: either side is accepted there."""
    rtol, atol = TOL["weights"]
    thr = float(MASK_THRESHOLD)
    return np.abs(np.asarray(w_ref, F64) - thr) <= atol + rtol * thr


# ---- float32 restatements in the kernels' order ----------------------------------------------------------------------------------
FAULTS = (None, "carry_shift", "no_segment_carry")  # the two wrong carries tests/test_render_cpu.py shows the closed forms to catch


def _alpha32(delta, sigma, density_scale, active):
    """alpha_of.  expf is restated as the correctly rounded exponential (float64 exp, rounded to fp32): numpy's own float32 exp
    depends on the SIMD path of the machine that runs it (up to 1.4 ulp where this was written: 8.4e-8 on the weights), and a
    measurement that a tolerance is derived from has to be the same everywhere.  One ulp of exp below 1 is 6e-8."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = ((F32(-2.0) * delta) * F32(density_scale)) * sigma if active else ((-delta) * F32(density_scale)) * sigma
        assert e.dtype == F32
        a = F32(1.0) - np.exp(e.astype(F64)).astype(F32)
    assert a.dtype == F32
    return a


def _scan(v, op):
    """Hillis-Steele over the 64 lanes of [N,64]: wave_excl_scan_mul / wave_excl_scan_add.  -> (exclusive, total [N])."""
    inc, d = v.copy(), 1
    while d < CHUNK:
        nxt = inc.copy()
        nxt[:, d:] = op(inc[:, d:], inc[:, :-d])
        inc, d = nxt, d * 2
    first = np.ones_like(v[:, :1]) if op is np.multiply else np.zeros_like(v[:, :1])
    return np.concatenate([first, inc[:, :-1]], axis=1), inc[:, -1].copy(), inc


def _wave_sum(v):
    lanes, d = np.arange(CHUNK), CHUNK // 2
    while d > 0:
        v = v + v[:, lanes ^ d]
        d //= 2
    return v[:, 0].copy()


def _chunks(T):
    """[(segment index, first sample, samples in the chunk)] in the forward kernel's order."""
    return [(j0 // SEGMENT, j0, min(CHUNK, T - j0)) for j0 in range(0, T, CHUNK)]


def _lanes(a, j0, n, fill):
    out = np.full((a.shape[0], CHUNK), fill, F32)
    out[:, :n] = a[:, j0:j0 + n]
    return out


def _delta32(z, sample_dist):
    return np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], F32(sample_dist))], axis=1)


def composite_fwd_f32(sigma, z, sample_dist, density_scale, active, fault=None):
    """composite_fwd_kernel in numpy float32.  -> dict(weights, weights_sum, depth, mask)."""
    assert sigma.dtype == z.dtype == F32 and fault in FAULTS
    N, T = z.shape
    alpha = _alpha32(_delta32(z, sample_dist), sigma, density_scale, active)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        fac = (F32(1.0) - alpha) + EPS_T
        w = np.zeros((N, T), F32)
        carry = np.ones(N, F32)
        wsum, dsum = np.zeros((N, CHUNK), F32), np.zeros((N, CHUNK), F32)
        seg_now = 0
        for seg, j0, n in _chunks(T):
            if seg != seg_now and fault == "no_segment_carry":
                carry = np.ones(N, F32)
            seg_now = seg
            ex, total, inc = _scan(_lanes(fac, j0, n, 1.0), np.multiply)
            tr = carry[:, None] * ex
            carry = carry * (inc[:, -2] if fault == "carry_shift" else total)
            wk = _lanes(alpha, j0, n, 0.0) * tr
            w[:, j0:j0 + n] = wk[:, :n]
            wsum[:, :n] = wsum[:, :n] + wk[:, :n]
            dsum[:, :n] = dsum[:, :n] + wk[:, :n] * z[:, j0:j0 + n]
        out = dict(weights=w, weights_sum=_wave_sum(wsum), depth=_wave_sum(dsum), mask=(w > MASK_THRESHOLD).astype(np.uint8))
    assert w.dtype == out["depth"].dtype == F32
    return out


def composite_image_f32(weights, attr, C):
    """composite_image_kernel: lane sums over j = lane, lane + 64, ..., then the butterfly."""
    N, T = weights.shape
    a = attr.reshape(N, T, C)
    out = np.empty((N, C), F32)
    for ch in range(C):
        s = np.zeros((N, CHUNK), F32)
        for j0 in range(0, T, CHUNK):
            n = min(CHUNK, T - j0)
            s[:, :n] = s[:, :n] + weights[:, j0:j0 + n] * a[:, j0:j0 + n, ch]
        out[:, ch] = _wave_sum(s)
    return out


def composite_bwd_f32(sigma, z, weights, attr, C, sample_dist, density_scale, active, d_depth, d_wsum, d_image, d_weights,
                      fault=None):
    """composite_bwd_kernel in numpy float32: the segment products' pass, then per segment from the far end the forward pass of
    the chunks and the backward pass with the suffix carry.  None = null pointer.  -> d_sigma [N,T], d_attr [N*T,C]."""
    assert sigma.dtype == z.dtype == weights.dtype == F32 and fault in FAULTS and C <= C_MAX and z.shape[1] <= T_MAX
    N, T = z.shape
    delta = _delta32(z, sample_dist)
    alpha = _alpha32(delta, sigma, density_scale, active)
    gd = d_depth if d_depth is not None else np.zeros(N, F32)
    gs = d_wsum if d_wsum is not None else np.zeros(N, F32)
    gi = d_image if d_image is not None else np.zeros((N, C), F32)
    kappa = F32(2.0 if active else 1.0)
    a3 = None if attr is None else attr.reshape(N, T, C)
    nseg = (T + SEGMENT - 1) // SEGMENT
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        fac = (F32(1.0) - alpha) + EPS_T
        seg_in, carry = [], np.ones(N, F32)
        for s in range(nseg):
            seg_in.append(np.ones(N, F32) if fault == "no_segment_carry" else carry)
            if s + 1 >= nseg:
                break
            prod = np.ones((N, CHUNK), F32)
            for j0 in range(s * SEGMENT, min(T, (s + 1) * SEGMENT), CHUNK):
                prod = prod * _lanes(fac, j0, min(CHUNK, T - j0), 1.0)
            carry = carry * _scan(prod, np.multiply)[1]
        d_sigma = np.zeros((N, T), F32)
        suffix_carry = np.zeros(N, F32)
        for s in range(nseg - 1, -1, -1):
            chunks = [(j0, min(CHUNK, T - j0)) for j0 in range(s * SEGMENT, min(T, (s + 1) * SEGMENT), CHUNK)]
            carry, trv = seg_in[s], []
            for j0, n in chunks:
                ex, total, inc = _scan(_lanes(fac, j0, n, 1.0), np.multiply)
                trv.append(carry[:, None] * ex)
                carry = carry * (inc[:, -2] if fault == "carry_shift" else total)
            for (j0, n), tr in reversed(list(zip(chunks, trv))):
                sl = slice(j0, j0 + n)
                g = gd[:, None] * z[:, sl] + gs[:, None]
                if d_weights is not None:
                    g = g + d_weights[:, sl]
                if a3 is not None:
                    for ch in range(C):
                        g = g + gi[:, None, ch] * a3[:, sl, ch]
                q = np.zeros((N, CHUNK), F32)
                q[:, :n] = g * weights[:, sl]
                before, qtotal, _ = _scan(q, np.add)
                suf = ((qtotal[:, None] - before) - q) + suffix_carry[:, None]
                a = alpha[:, sl]
                da = g * tr[:, :n] - suf[:, :n] / ((F32(1.0) - a) + EPS_T)
                d_sigma[:, sl] = da * (((kappa * delta[:, sl]) * F32(density_scale)) * (F32(1.0) - a))
                suffix_carry = suffix_carry + qtotal
        d_attr = None if not C else (weights[:, :, None] * gi[:, None, :]).reshape(N * T, C)
    assert d_sigma.dtype == F32
    return d_sigma, d_attr
