"""Float64 reference, inputs, bounds and route map for the exact tests of the fused field encode (csrc/fused.hip) and its adjoint
(csrc/field_bwd.hip): tests/test_field_cpu.py, tests/test_gpu_field_exact.py.  numpy / CPU torch only: importable without a device,
and nothing here is computed by HIP code.  The planes half is tests/planes_width_ref.py (``density_fwd`` / ``density_bwd``, pinned
against the oracle by tests/test_planes_width_cpu.py), the hash half is tests/hashgrid_cases.py (``Geom``, ``level_corners``,
``fwd_ref``, ``t_fwd_ref``, ``t_expand_ref``, the slice pair and the Lagrange basis), both by import; what is new here is their
composition as ``oracle/fields_ref.py: LiDAR4D.density`` (lines 341-365) composes them, the analytic adjoint of that composition, the
bounds below and the restatement of the host logic that picks the kernels.

WHAT THE REFERENCE SAYS (``encode_ref``, ``encode_adjoint_ref``)
  row        [planes_s | planes_d | hash_s | hash_d | 1 ... 1]: columns from the field width to in_pad are 1.0 (tiny-cuda-nn pads the
             network input with ones).
  blend      0.5 * f(x, t) + 0.25 * (f(x + flow_fwd, t1) + f(x + flow_bwd, t2)).  A neighbour that does not exist (first / last frame)
             is REPLACED BY THE CURRENT FRAME'S VALUE, WITH ITS GRADIENT: the current frame's weight c0 is 0.5, 0.75 or 1.0.
  no_grad    the two flow-warped HASH lookups sit under torch.no_grad() in the reference model (fields_ref.py:354,360).  Hash tables
             therefore receive gradient through the current frame's term ONLY (with weight c0, the warped terms being constants), and
             d(flow) comes from the time planes ALONE.  A test that differentiates through the warped hash lookups would be wrong.
  copies     inputs are what the kernels receive: fp16 hash tables, fp32 planes, fp16 flow; x + flow is the fp32 sum.  The cell a
             plane coordinate falls into and its clip mask come from the fp32 position arithmetic (planes_width_ref.py's rule); every
             slice feature of a 2-D x time stack is rounded to fp16 before the time blend (tiny-cuda-nn's rounding point R2, which the
             oracle has in its "tcnn" mode); everything else is float64.
  time       ``tinfo`` is given literally (planes_width_ref.time_info, with the reference's /num_frames quirk).
  dflow16    columns 6 .. 15 are +0; dflow16 is NOT multiplied by param_scale (it stays in dX's loss-scaled domain).

HOW THE KERNELS ARE JUDGED.  u = 2^-24 (one fp32 rounding, relative).  The coordinates of every cloud are multiples of 1/16 (the
lattice of hashgrid_cases.py; the ray clouds of the band-skip cases: multiples of 1/1024), tables hold integers in [-8, 8].

  hash_s columns (class L)    every term exact in fp32 in any order: fp16(float64), bit for bit, on every route (gathered with and
                              without pair loads, level-major inside the LDS kernel and as a launch of its own).
  hash_d columns (class E)    slice features exact, rounded to fp16; blend w1 a + w2 b, r += basis[f] * (.), and
                              0.5 r0 + 0.25 (r1 + r2) in numpy float32 in the order fused.hip / field_dev.h write them (the file is
                              compiled without contraction; pair_eval's fmix0 products are single roundings of the same products).
                              Bit for bit.  test_field_cpu.py checks that this emulation lies within 8 u sum|terms| of ``encode_ref``.
  plane columns               accepted: fp16(float64 value v); or, where v lies within E of an fp16 rounding midpoint, the fp16 value
                              on the other side.  E per element, counted along planes_dev.h / fused.hip:
                                position   p = ((2 c - 1) + 1) / 2 * (size - 1) is fp32 by the sampler's definition; the reference
                                           takes the cell from it and the weights from float64: dp = |p_fp32 - p_float64| exactly
                                           (0 on the lattice), weights w1 = p - floor p, w0 = (floor p + 1) - p are exact in fp32;
                                tap        v_j = ((a nw + b ne) + c sw) + d se: weight product, tap product, three adds = 5 u max|tap|
                                           (the 1-D row route: 2 + 2 roundings), plus slope_x dp_x + slope_y dp_y
                                           = e_j;
                                product    (v0 v1) v2: 2 u |v0 v1 v2| + sum_j e_j prod_{k != j} |v_k|        = E_g (static: E = E_g);
                                blend      0.5 d0 + 0.25 (d1 + d2): 0.5 E_g0 + 0.25 (E_g1 + E_g2) + u 0.25 |d1 + d2| + u |result|.
                              all times (1 + 2^-20) for the second-order terms.  Condition (test_field_cpu.py): at most 1 % of a
                              case's plane elements lie that close to a midpoint.  Measured: 0.30 - 0.47 %.
  static table gradient       sorted scatter (binscatter.hip) on levels that are not binned (2^11 entries: one bin): run-merged fp32
                              atomics of lattice values, class L, bit for bit, prefill included.
  slice table gradients       lattice clouds: gdynT = fp16(dX c0) exact, go * w * 2^k an integer, int64 sum exact, H exact in fp32;
                              then h = H * param_scale, g += (h * basis[f]) * w in numpy float32 (class E, hashgrid_cases.t_expand_ref):
                              bit for bit; the slices outside the blended pair keep their bits.
                              ray clouds (multiples of 1/1024: H is not an fp32 number): bound
                                |basis w param_scale| * [(W + 1) u sum|c|] + 3 u |term| + u (|g0| + |term|),   W = workgroups per task.
  plane gradients             per element, A = sum |c_k| over the n contributions c_k = corner weight * upstream * other planes' values:
                                static   gvs = fp16(g va vb)                                       2^-11 A
                                         va, vb sampled in fp32 (5 u each), two products, the weight product, gv * w, four scan
                                         steps of a merged run, int -> float, * (param_scale / scale)    20 u A
                                         fx_scale(chunk * max|gvs| * 1.01, 30): quantum q <= 2.02 chunk max|gvs| 2^-30, half of it
                                         per fx_round, at most one per contribution                n q / 2
                                         one fp32 atomic per workgroup onto the running value      W u (|g0| + param_scale A)
                                time     as above without the fp16 term (dX is fp16 already), 22 u A (three products, row weight at
                                         the flush), q <= 2.02 chunk max|gd| vmax^2 2^-30 applied with the row weight wy at the flush:
                                         sum_k wy_k q / 2;  W = chunks * frames present.
                                both     + A_pos = sum |g v v| (dp_x + dp_y): the corner weights the kernel takes from p_fp32.
                              No margin.  Condition (test_field_cpu.py): at least 95 % of the non-zero contributions exceed twice
                              their element's bound.  Measured: 99.99 - 100 % on the lattice clouds; ray clouds 99.3 % (2,048 rows), 98.8 % (4,096),
                              97.3 % (71,680, see ``band_case``).
  dflow16                     fp16 of an fp32 dot product (contraction allowed there): per (frame, axis)
                                d = sum_{s, k} [ 24 u |dv_k gv_k| + 8 u M |gv_k| ] * mult,  M = max |time plane value| of the scale,
                              then |got - ref| <= d + 2^-11 (|ref| + d) + 2^-25.

Every route the library launches is selected by its arguments, and the route map below (``fwd_routes``, ``bwd_routes``) is complete.

Largest |error| / bound observed on an MI355X (printed by test_gpu_field_exact.py): OBSERVED below.  They are observations, not
inputs to the bounds.
"""
import functools

import numpy as np
import torch

import hashgrid_cases as hc
import planes_width_ref as pw
from glue_cases import F16, F32, F64, rng_of, same_bits, to_f32_exact  # noqa: F401 (re-exported)

U = 2.0 ** -24
T64 = torch.float64
OBSERVED = """
    static planes   0.99 (lattice clouds)   0.88 (ray clouds)     -- the fp16 payload of gvs: an element with one contribution sits at
                                                                     up to 2^-11 of it, which is the bound
    time planes     0.47                    0.29
    dflow16         0.97                                          -- its last step is a rounding to fp16: 2^-11 |value| is reached
    slice tables    bit for bit             1.00 (ray clouds)     -- the fp32 add onto a prefill that is a power of two
    static table, hash_s, hash_d columns, slice tables on the lattice: bit for bit.  Plane columns: every element fp16(float64) or
    the fp16 value across a midpoint within E.
"""
AXES = ((0, 1), (0, 2), (1, 2))  # xy, xz, yz
# (x, y, z, t) per scale.  x, y, z differ in the first scale (a swapped axis shows) and every lattice z is a texel centre of its 65 rows;
# the second scale's xy plane is 64 x 64: two 64 KB row bands (the others: two or three, the last one ragged).  No static plane has
# fewer than 3,640 texels: with 71,680 samples on a 16 x 16 plane the fp16 term of a texel's bound would exceed its contributions.
PLANE_RES = ((56, 72, 65, 5), (64, 64, 80, 7))
FULL = 4161  # coprime to 64 and 512: repeated, every point meets every lane position
ENC_HS_PRE_MIN_POINTS = 1 << 18
DH_MAX_ENTRIES = 8192


# ---- the field -------------------------------------------------------------------------------------------------------------------
class FieldSpec:
    """What the GPU test builds its l4d_field_desc from: 2 plane scales, a static 3-D grid of ``Ls`` levels (2^11 entries: no level
    binned by the sorted scatter), xy / xz / yz stacks of ``Ld`` levels (2^15 / 2^13 / 2^13 entries unless ``log2T_d`` says otherwise:
    the forward's LDS kernel takes xz / yz tables of at most 2^13), 8 slices.  Base resolution 3, per-level scale 2 (hashgrid_cases.Geom)."""

    def __init__(self, Ls, Ld, log2T_d=None, n_slices=8, plane_res=PLANE_RES):
        self.Ls, self.Ld, self.n_slices, self.plane_res = Ls, Ld, n_slices, tuple(plane_res)
        self.log2T_d = tuple(log2T_d or (15, 13, 13))
        self.hs = hc.Geom(3, 4, 11, Ls)
        self.hd = [hc.Geom(2, 4, l2, Ld) for l2 in self.log2T_d]
        self.n_scales, self.C = len(self.plane_res), 8
        self.plane_off, off = [], 0
        for s in range(self.n_scales):
            for ci in range(6):
                H, W = self.plane_shape(s, ci)
                self.plane_off.append(off)
                off += H * W * self.C
        self.plane_numel = off
        self.colsA = 2 * self.n_scales * self.C
        self.colD = self.colsA + 4 * Ls
        self.L3 = 3 * Ld
        self.width = self.colD + self.L3
        self.key = (Ls, Ld) + self.log2T_d

    def plane_shape(self, s, ci):
        a, b = pw.COMBS[ci]
        return self.plane_res[s][b], self.plane_res[s][a]  # H, W

    def plane_slice(self, s, ci):
        H, W = self.plane_shape(s, ci)
        o = self.plane_off[s * 6 + ci]
        return slice(o, o + H * W * self.C)


# 8: xy levels 0 .. 4 dense (16 .. 2,304 entries), 5 dense and larger than one 64 KB window (9,216), 6 and 7 hashed 2^15 (parity tasks);
# xz / yz: 5 .. 7 hashed 2^13 (one window).  "6/8": unequal level counts, xy 2^16: level 6 dense 36,864 (three ranges), 7 hashed (four).
SPECS = {4: FieldSpec(4, 4), 8: FieldSpec(8, 8), 16: FieldSpec(16, 16, log2T_d=(13, 13, 13)), "6/8": FieldSpec(6, 8, log2T_d=(16, 13, 13))}


def params_of(spec):
    """Deterministic parameters of a spec (made once per spec object): planes in the ranges the model starts from
    (planes_width_ref.fill_planes), integer tables."""
    if getattr(spec, "_params", None) is None:
        planes = []
        for s in range(spec.n_scales):
            coefs = []
            for ci in range(6):
                H, W = spec.plane_shape(s, ci)
                lo, hi = (0.75, 1.25) if ci in pw.TIME else (0.1, 0.5)
                coefs.append(torch.from_numpy((lo + (hi - lo) * rng_of(67, s, ci, H, W).rand(1, spec.C, H, W)).astype(F32)))
            planes.append(coefs)
        k = [int(v) for v in spec.key]
        hs_table = hc.table_values(spec.hs.n_entries * 4, 101, *k)
        hd_tables = [[hc.table_values(g.n_entries * 4, 103, p, s, *k) for s in range(spec.n_slices)] for p, g in enumerate(spec.hd)]
        spec._params = dict(planes=planes, hs_table=hs_table, hd_tables=hd_tables)
    return spec._params


def to_arena(spec, planes, dtype=F32):
    """Channel-last arena [H][W][C] per plane at spec.plane_off."""
    out = np.zeros(spec.plane_numel, dtype)
    for s in range(spec.n_scales):
        for ci in range(6):
            out[spec.plane_slice(s, ci)] = planes[s][ci][0].permute(1, 2, 0).reshape(-1).numpy().astype(dtype)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def frame_info(frame, num_frames):
    """-> (t fp32, tinfo of planes_width_ref.time_info, tinfo8: the eight floats of l4d_time_setup)."""
    t = F32(frame / (num_frames - 1))
    assert int(t * F32(num_frames - 1)) == frame
    ti = pw.time_info(t, num_frames)
    return t, ti, np.array([ti[0], ti[1], ti[2], float(ti[3]), float(ti[4]), float(frame), 0.0, 0.0], F32)


FRAMES = ((0, 51), (22, 51), (25, 51), (50, 51), (0, 2), (1, 2))  # (22: the backward neighbour's time lies on another slice pair)


@functools.lru_cache(maxsize=None)
def _cloud_full(key):
    x = hc.lattice_points(FULL, 3, 211, key)
    plant = np.array([[0, 0, 0], [16, 16, 16], [-1, -1, -1], [17, 17, 17], [-1, 17, 0], [16, -1, 17], [0, 16, -1], [8, 8, 8]], F64)
    x[:8] = (plant / 16.0).astype(F32)
    fl = rng_of(223, key).randint(-3, 4, size=(FULL, 6)).astype(F64) / 16.0
    fl[0], fl[1] = -2.0 / 16.0, 2.0 / 16.0  # the warped points leave [0, 1] across the border
    fl[7] = 0.0                              # a warped point that stays where the sample is
    flow16 = np.full((FULL, 16), np.nan, F16)  # columns 6 .. 15 are never read
    flow16[:, :6] = fl.astype(F16)
    return x, flow16


def cloud(P, t, key=0):
    """xt [P, 4] fp32 and flow16 [P, 16] fp16: the first P rows of one lattice cloud of FULL points, repeated beyond that."""
    x, flow16 = _cloud_full(key)
    rows = np.arange(P) % FULL
    xt = np.empty((P, 4), F32)
    xt[:, :3], xt[:, 3] = x[rows], t
    return xt, flow16[rows].copy()


def ray_cloud(n_rays, t, key=0, T=64):
    """Rays of T = 64 samples on the lattice of 1/1024: along a ray every coordinate is rising, falling or constant; the first rays
    start and end exactly on the band edge of the 64 x 64 plane (row 32 of 64: coordinate 32 / 63 is no lattice value, so the nearest
    rows: y from just below to just above, one row inside and one outside)."""
    r = rng_of(227, n_rays, key)
    a = r.randint(0, 1025 - 4 * T, size=(n_rays, 3))
    step = r.randint(0, 5, size=(n_rays, 3)) * np.where(r.rand(n_rays, 3) < 0.5, -1, 1)
    k = np.arange(T)[None, :, None]
    start = np.where(step < 0, a + 4 * T, a)[:, None, :]
    q = start + step[:, None, :] * k  # [n, T, 3], in 0 .. 1024
    # ray 0: y constant between rows 30 and 31 (band 0 only); ray 1: y constant in row 32 (band 1 only); ray 2: y from row 31 up into row 32
    q[0, :, 1], q[1, :, 1] = 496, 521   # 496 / 1024 * 63 = 30.5 (rows 30, 31), 521 / 1024 * 63 = 32.05 (rows 32, 33)
    q[2, :, 1] = 504 + np.arange(T) // 4  # 31.01 .. 31.93 ... stays below 32: taps rows 31 and 32 -> both bands
    x = (q.reshape(-1, 3).astype(F64) / 1024.0).astype(F32)
    xt = np.empty((n_rays * T, 4), F32)
    xt[:, :3], xt[:, 3] = x, t
    fl = r.randint(-3, 4, size=(n_rays * T, 6)).astype(F64) / 16.0
    flow16 = np.full((n_rays * T, 16), np.nan, F16)
    flow16[:, :6] = fl.astype(F16)
    return xt, flow16


def make_dX(spec, P, in_pad, key=0, hash_cols=True, sparse_planes=0.0):
    """fp16 [P, in_pad]: plane columns fp16 values of magnitude 0.25 .. 1 and either sign, hash columns multiples of 1/4 in [-2, 2] (static grid: in [-1, 1]; zero where not wanted), a tenth
    of the rows and the wavefront of rows 128 .. 191 zero, padding columns NaN (never read).  sparse_planes: that share of the rows
    has zero plane columns and the time-plane columns are zero in every row (the 71,680-row case, see ``band_case``)."""
    r = rng_of(229, P, in_pad, key)
    d = np.full((P, in_pad), np.nan, F16)
    d[:, :spec.colsA] = ((0.25 + 0.75 * r.rand(P, spec.colsA)) * np.where(r.rand(P, spec.colsA) < 0.5, -1.0, 1.0)).astype(F16)
    d[:, spec.colsA:spec.width] = (r.randint(-8, 9, size=(P, spec.width - spec.colsA)) / 4.0).astype(F16) if hash_cols else 0.0
    if hash_cols:  # (static grid: [-1, 1], so that its coarsest level's sums stay below 2^24 lattice units)
        d[:, spec.colsA:spec.colD] = (r.randint(-4, 5, size=(P, spec.colD - spec.colsA)) / 4.0).astype(F16)
    zero = r.rand(P) < 0.1
    zero[128:192] = True
    d[zero, :spec.width] = 0.0
    if sparse_planes:
        d[r.rand(P) < sparse_planes, :spec.colsA] = 0.0
        d[:, spec.colsA // 2:spec.colsA] = 0.0
    return d


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def _tensors(xt, flow16):
    return torch.from_numpy(np.ascontiguousarray(xt)), torch.from_numpy(flow16[:, :6].astype(F32))


def frame_coords(xt, flow16, tinfo):
    """[(x [P, 3] fp32, t, present)] of the three lookups; x + flow is the fp32 sum."""
    t0, t1, t2, has_fwd, has_bwd = tinfo
    x, fl = xt[:, :3].astype(F32), flow16[:, :6].astype(F32)
    return [(x, t0, True), ((x + fl[:, :3]).astype(F32), t1, bool(has_fwd)), ((x + fl[:, 3:6]).astype(F32), t2, bool(has_bwd))]


def _t_fwd64(geom, x2, tables, t):
    """One 2-D x time stack at time t in float64: slice features fp16(exact), blend, Lagrange basis (weights and basis are the fp32
    numbers the model computes from t, used as float64)."""
    L = geom.n_levels
    i1, i2, w1, w2 = hc.slice_pair_f32(t, len(tables))
    basis = hc.lagrange4_f32(t).astype(F64)
    a = hc.fwd_ref(geom, x2, tables[i1])[1].astype(F64)
    if i1 != i2:
        a = float(w1) * a + float(w2) * hc.fwd_ref(geom, x2, tables[i2])[1].astype(F64)
    return (a.reshape(-1, L, 4) * basis[None, None, :]).sum(2)


def dyn_cols(spec, params, xt, flow16, tinfo, emulate):
    """hash_d [P, 3 Ld]: float64, or (emulate) the fp32 values in the order fused.hip computes them."""
    fr = frame_coords(xt, flow16, tinfo)
    out = []
    for p, geom in enumerate(spec.hd):
        ax = list(AXES[p])
        if emulate:
            r = [hc.t_fwd_ref(geom, np.ascontiguousarray(x[:, ax]), params["hd_tables"][p], t) if ok else None for x, t, ok in fr]
            r1, r2 = (r[1] if r[1] is not None else r[0]), (r[2] if r[2] is not None else r[0])
            v = F32(0.5) * r[0] + F32(0.25) * (r1 + r2)
            assert v.dtype == F32
        else:
            r = [_t_fwd64(geom, np.ascontiguousarray(x[:, ax]), params["hd_tables"][p], t) if ok else None for x, t, ok in fr]
            r1, r2 = (r[1] if r[1] is not None else r[0]), (r[2] if r[2] is not None else r[0])
            v = 0.5 * r[0] + 0.25 * (r1 + r2)
        out.append(v)
    return np.concatenate(out, 1)


def encode_ref(spec, params, xt, flow16, tinfo, in_pad):
    """The float64 row [planes_s | planes_d | hash_s | hash_d | 1 ... 1] of LiDAR4D.density (module docstring)."""
    P = xt.shape[0]
    row = np.ones((P, in_pad), F64)
    xt_t, fl_t = _tensors(xt, flow16)
    ps, pd = pw.density_fwd(params["planes"], xt_t, fl_t, tinfo)
    n = spec.n_scales * spec.C
    row[:, :n], row[:, n:2 * n] = ps.numpy(), pd.numpy()
    row[:, spec.colsA:spec.colD] = hc.fwd_ref(spec.hs, np.ascontiguousarray(xt[:, :3]), params["hs_table"])[0]
    row[:, spec.colD:spec.width] = dyn_cols(spec, params, xt, flow16, tinfo, emulate=False)
    return row


def _dp(c32, size):
    """|p_fp32 - p_float64| of the sampler's position (both clamped to the plane)."""
    hi = float(size - 1)
    p32 = (((c32 * 2.0 - 1.0) + 1.0) / 2.0 * hi).clamp(0.0, hi)
    p64 = (((c32.to(T64) * 2.0 - 1.0) + 1.0) / 2.0 * hi).clamp(0.0, hi)
    return (p32.to(T64) - p64).abs()


def _group_eps(group, coords):
    """E_g [P, C] of one product of three planes (module docstring)."""
    eps = []
    for ci, tap in zip(group.cis, group.taps):
        _, H, W = tap.shape
        v00, v01, v10, v11 = tap.v
        m = torch.stack([v.abs() for v in tap.v]).max(0).values
        sx = torch.maximum((v01 - v00).abs(), (v11 - v10).abs())
        sy = torch.maximum((v10 - v00).abs(), (v11 - v01).abs())
        dpx, dpy = _dp(coords[:, pw.COMBS[ci][0]], W), _dp(coords[:, pw.COMBS[ci][1]], H)
        eps.append(5.0 * U * m + sx * dpx.unsqueeze(1) + sy * dpy.unsqueeze(1))
    v = [t.val.abs() for t in group.taps]
    return 2.0 * U * group.prod.abs() + eps[0] * v[1] * v[2] + eps[1] * v[0] * v[2] + eps[2] * v[0] * v[1]


def plane_eps(spec, params, xt, flow16, tinfo):
    """E [P, 2 n_scales C]: the absolute fp32 bound of the plane columns."""
    xt_t, fl_t = _tensors(xt, flow16)
    (c0, _), (c1, has_fwd), (c2, has_bwd) = pw._frames(xt_t, fl_t, tinfo)
    es, ed = [], []
    for coefs in params["planes"]:
        es.append(_group_eps(pw._Group(coefs, c0, False), c0))
        g0 = pw._Group(coefs, c0, True)
        g1 = pw._Group(coefs, c1, True) if has_fwd else g0
        g2 = pw._Group(coefs, c2, True) if has_bwd else g0
        e0 = _group_eps(g0, c0)
        e1 = _group_eps(g1, c1) if has_fwd else e0
        e2 = _group_eps(g2, c2) if has_bwd else e0
        pd = 0.5 * g0.prod + 0.25 * (g1.prod + g2.prod)
        ed.append(0.5 * e0 + 0.25 * (e1 + e2) + U * 0.25 * (g1.prod + g2.prod).abs() + U * pd.abs())
    return torch.cat(es + ed, 1).numpy() * (1.0 + 2.0 ** -20)


def f16_accept(v64, eps):
    """-> (want fp16(v64), other: the fp16 value across the nearest rounding midpoint, near: v64 within eps of that midpoint)."""
    from glue_cases import _f16_ext
    v = np.asarray(v64, F64)
    want = v.astype(F16)
    a = np.abs(v)
    wb = np.abs(want).view(np.uint16).astype(np.int64)
    w = _f16_ext(wb)
    up = a >= w
    ob = np.where(up, wb + 1, np.maximum(wb - 1, 0))
    mid = 0.5 * (w + _f16_ext(ob))
    near = (np.abs(a - mid) <= eps) & (ob != wb)
    other = (np.minimum(ob, 0x7C00) | np.where(np.signbit(v), 0x8000, 0)).astype(np.uint16).view(F16)
    return want, other, near


@functools.lru_cache(maxsize=None)
def fwd_case(spec_name, frame, num_frames, key=0):
    """Reference rows of the FULL-point cloud, computed once: a smaller cloud is its first rows, a larger one repeats it."""
    spec = SPECS[spec_name]
    params = params_of(spec)
    t, tinfo, tinfo8 = frame_info(frame, num_frames)
    xt, flow16 = cloud(FULL, t, key)
    row = encode_ref(spec, params, xt, flow16, tinfo, spec.width)  # (the ones behind the width: ``padded``)
    nA = spec.colsA
    want, other, near = f16_accept(row[:, :nA], plane_eps(spec, params, xt, flow16, tinfo))
    want16 = row.astype(F16)
    want16[:, :nA] = want
    want16[:, spec.colD:spec.width] = dyn_cols(spec, params, xt, flow16, tinfo, emulate=True).astype(F16)
    other16 = want16.copy()
    other16[:, :nA] = other
    near_full = np.zeros(want16.shape, bool)
    near_full[:, :nA] = near
    return dict(spec=spec, params=params, t=t, tinfo=tinfo, tinfo8=tinfo8, xt=xt, flow16=flow16, row=row, want16=want16, other16=other16,
                near=near_full, near_share=float(near.mean()))


def padded(a, in_pad, fill):
    """[P, width] -> [P, in_pad] with ``fill`` in the padding columns."""
    out = np.full((a.shape[0], in_pad), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


# ---- adjoint ---------------------------------------------------------------------------------------------------------------------
def blend_c0(tinfo):
    return 0.5 + (0.0 if tinfo[3] else 0.25) + (0.0 if tinfo[4] else 0.25)


def _scatter1(geom, x2, g64):
    """H [n_entries] = sum of corner weight * g64[:, level] in float64, with sum |.|."""
    tot, mag, _ = hc.scatter64(geom, x2, g64, 1, want_abs=True)
    return tot, mag


def encode_adjoint_ref(spec, params, xt, flow16, tinfo, in_pad, dX, param_scale):
    """Analytic adjoint in float64 -> (plane gradients as a channel-last arena, static table gradient [n * 4], slice table gradients
    [plane][slice][n * 4], dflow [P, 6]).  Hash tables: the current frame's term only, weight c0 (the warped lookups are no_grad);
    dflow: from the time planes alone, not multiplied by param_scale."""
    dX64 = np.asarray(dX[:, :spec.width], F64)
    n = spec.n_scales * spec.C
    xt_t, fl_t = _tensors(xt, flow16)
    grads, dflow, _ = pw.density_bwd(params["planes"], xt_t, fl_t, tinfo, torch.from_numpy(dX64[:, :n]), torch.from_numpy(dX64[:, n:2 * n]))
    arena = to_arena(spec, grads, F64) * float(param_scale)
    x3 = np.ascontiguousarray(xt[:, :3])
    hs = hc.scatter64(spec.hs, x3, dX64[:, spec.colsA:spec.colD] * float(param_scale), 4)[0]
    c0 = blend_c0(tinfo)
    i1, i2, w1, w2 = hc.slice_pair_f32(tinfo[0], spec.n_slices)
    basis = hc.lagrange4_f32(tinfo[0]).astype(F64)
    hd = []
    for p, geom in enumerate(spec.hd):
        cols = slice(spec.colD + p * spec.Ld, spec.colD + (p + 1) * spec.Ld)
        H, _ = _scatter1(geom, np.ascontiguousarray(x3[:, list(AXES[p])]), dX64[:, cols] * c0)
        g = [np.zeros(geom.n_entries * 4) for _ in range(spec.n_slices)]
        for i, w in ((i1, w1), (i2, w2)) if i1 != i2 else ((i1, w1),):
            g[i] = (H[:, None] * basis[None, :] * float(w) * float(param_scale)).reshape(-1)
        hd.append(g)
    return arena, hs, hd, dflow.numpy()


def slice_grads_expected(spec, xt, tinfo, dX, param_scale, grads0):
    """Class E (lattice clouds): what every slice table holds afterwards, fp32 bit patterns.  Asserts that H is exact."""
    c0 = blend_c0(tinfo)
    x3 = np.ascontiguousarray(xt[:, :3])
    out = []
    for p, geom in enumerate(spec.hd):
        cols = slice(spec.colD + p * spec.Ld, spec.colD + (p + 1) * spec.Ld)
        g = np.asarray(dX[:, cols], F64) * c0
        assert (g.astype(F16).astype(F64) == g).all(), "gdynT = fp16(dX c0) not exact"
        H, mag = _scatter1(geom, np.ascontiguousarray(x3[:, list(AXES[p])]), g)
        unit = geom.w_unit / 16.0
        assert (H / unit == np.rint(H / unit)).all() and (mag / unit < hc.EXACT_SUM).all(), "H not exact in fp32"
        hs32 = to_f32_exact(H * float(param_scale), "H * param_scale")
        out.append(hc.t_expand_ref(geom, hs32, tinfo[0], grads0[p]))
    return out


def slice_grads_bound(spec, xt, tinfo, dX, param_scale, grads0, n_wg):
    """Ray clouds: (ref float64, bound) per plane and slice (module docstring)."""
    c0 = blend_c0(tinfo)
    x3 = np.ascontiguousarray(xt[:, :3])
    i1, i2, w1, w2 = hc.slice_pair_f32(tinfo[0], spec.n_slices)
    basis = hc.lagrange4_f32(tinfo[0]).astype(F64)
    out = []
    for p, geom in enumerate(spec.hd):
        cols = slice(spec.colD + p * spec.Ld, spec.colD + (p + 1) * spec.Ld)
        H, mag = _scatter1(geom, np.ascontiguousarray(x3[:, list(AXES[p])]), np.asarray(dX[:, cols], F64) * c0)
        per = []
        for s in range(spec.n_slices):
            g0 = grads0[p][s].astype(F64)
            w = float(w1) if s == i1 else float(w2) if (s == i2 and i1 != i2) else 0.0
            k = np.abs(basis[None, :] * w * float(param_scale))
            term = (H[:, None] * basis[None, :] * w * float(param_scale)).reshape(-1)
            bound = (k * ((n_wg + 1) * U * mag)[:, None]).reshape(-1) + 3 * U * np.abs(term) + U * (np.abs(g0) + np.abs(term))
            per.append((g0 + term, bound if w else np.zeros_like(term)))
        out.append(per)
    return out


def plane_adjoint_bounds(spec, params, xt, flow16, tinfo, dX, param_scale, route, g0_arena):
    """-> dict(bound: arena of per-element bounds, seen: share of the non-zero contributions above twice their element's bound,
    vmax, gd_max).  ``route``: bwd_routes(...) of the call (chunk sizes and workgroup counts)."""
    ps = float(param_scale)
    dX64 = np.asarray(dX[:, :spec.colsA], F64)
    n = spec.n_scales * spec.C
    xt_t, fl_t = _tensors(xt, flow16)
    frames = pw._frames(xt_t, fl_t, tinfo)
    c0 = blend_c0(tinfo)
    vmax = float(max(float(p.abs().max()) for coefs in params["planes"] for p in coefs))
    gd_all = torch.from_numpy(dX64[:, n:2 * n])
    gd_max = float(gd_all.abs().max()) if gd_all.numel() else 0.0
    q_t = 2.02 * route["chunk"] * gd_max * vmax * vmax * 2.0 ** -30 + 1e-30
    n_frames = 1 + int(bool(tinfo[3])) + int(bool(tinfo[4]))
    bound = np.zeros(spec.plane_numel)
    g0 = np.abs(np.asarray(g0_arena, F64))
    seen = total = 0
    for s, coefs in enumerate(params["planes"]):
        C = spec.C
        gs = torch.from_numpy(dX64[:, s * C:(s + 1) * C])
        gd = gd_all[:, s * C:(s + 1) * C]
        work = []  # (ci, [(idx, |c|, quantum weight)], kind)
        grp = pw._Group(coefs, frames[0][0], False)
        gvs_max = 0.0
        for j, (ci, tap) in enumerate(zip(grp.cis, grp.taps)):
            o = [t.val for i, t in enumerate(grp.taps) if i != j]
            gv = gs * o[0] * o[1]
            gvs_max = max(gvs_max, float(gv.abs().max()) if gv.numel() else 0.0)
            work.append((ci, tap, gv, frames[0][0], "s"))
        q_s = 2.02 * route["chunk_ps"] * gvs_max * (1.0 + 2.0 ** -10) * 2.0 ** -30 + 1e-30
        for e, (coords, present) in enumerate(frames):
            if not present:
                continue
            grp = pw._Group(coefs, coords, True)
            coef = c0 if e == 0 else 0.25
            for j, (ci, tap) in enumerate(zip(grp.cis, grp.taps)):
                o = [t.val for i, t in enumerate(grp.taps) if i != j]
                work.append((ci, tap, coef * gd * o[0] * o[1], coords, "t"))
        acc = {}
        for ci, tap, gv, coords, kind in work:
            _, H, W = tap.shape
            A, Q, Ap = acc.setdefault(ci, [torch.zeros(H * W, C, dtype=T64) for _ in range(3)])
            dp = (_dp(coords[:, pw.COMBS[ci][0]], W) + _dp(coords[:, pw.COMBS[ci][1]], H)).unsqueeze(1)
            wys = (tap.wy0, tap.wy0, tap.wy1, tap.wy1)
            for idx, w, wy in zip(tap.idx, tap.w, wys):
                c = (w.unsqueeze(1) * gv).abs()
                nz = (c != 0).to(T64)
                A.index_add_(0, idx, c)
                Q.index_add_(0, idx, nz * (0.5 * q_s if kind == "s" else wy.unsqueeze(1) * 0.5 * q_t))
                Ap.index_add_(0, idx, gv.abs() * dp * nz)
        for ci, (A, Q, Ap) in acc.items():
            sl = spec.plane_slice(s, ci)
            A, Q, Ap = (a.reshape(-1).numpy() for a in (A, Q, Ap))
            if ci in pw.STATIC:
                b = ps * ((2.0 ** -11 + 20 * U) * A + Q + Ap) + route["n_chunks_ps"] * U * (g0[sl] + ps * A)
            else:
                b = ps * (22 * U * A + Q + Ap) + route["n_chunks"] * n_frames * U * (g0[sl] + ps * A)
            bound[sl] = b
        for ci, tap, gv, coords, kind in work:
            _, H, W = tap.shape
            b = torch.from_numpy(bound[spec.plane_slice(s, ci)]).reshape(H * W, C)
            for idx, w in zip(tap.idx, tap.w):
                c = (w.unsqueeze(1) * gv).abs() * ps
                nz = c != 0
                seen += int((c[nz] > 2.0 * b[idx][nz]).sum())
                total += int(nz.sum())
    return dict(bound=bound, seen=seen / total if total else 1.0, vmax=vmax, gd_max=gd_max)


def dflow_bound(spec, params, xt, flow16, tinfo, dX, dflow_ref):
    """[P, 6] bound of dflow16 (module docstring)."""
    P = xt.shape[0]
    n = spec.n_scales * spec.C
    dX64 = np.asarray(dX[:, :spec.colsA], F64)
    xt_t, fl_t = _tensors(xt, flow16)
    frames = pw._frames(xt_t, fl_t, tinfo)
    d = torch.zeros(P, 6, dtype=T64)
    for s, coefs in enumerate(params["planes"]):
        gd = torch.from_numpy(dX64[:, n + s * spec.C:n + (s + 1) * spec.C])
        M = max(float(coefs[ci].abs().max()) for ci in pw.TIME)
        for e in (1, 2):
            coords, present = frames[e]
            if not present:
                continue
            grp = pw._Group(coefs, coords, True)
            for j, tap in enumerate(grp.taps):
                o = [t.val for i, t in enumerate(grp.taps) if i != j]
                gv = (0.25 * gd * o[0] * o[1]).abs()
                v00, v01, v10, v11 = tap.v
                dv = ((v01 - v00) * tap.wy0.unsqueeze(1) + (v11 - v10) * tap.wy1.unsqueeze(1)).abs()
                d[:, (e - 1) * 3 + j] += ((24 * U * dv * gv + 8 * U * M * gv).sum(1)) * tap.mx
    d = d.numpy()
    return d + 2.0 ** -11 * (np.abs(dflow_ref) + d) + 2.0 ** -25


# ---- the host logic that picks the kernels, restated -------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def pair_ok(spec, table_aligned16):
    return bool(table_aligned16 and all(o % 2 == 0 for o in spec.hs.offset))


def fwd_routes(spec, P, scratch, rows, table_aligned16=True, sigma=None):
    """encode_fwd_impl (fused.hip): the launches of one call.  sigma: None or (in_pad, n_hidden)."""
    if P == 0:
        return dict(kernels=[])
    k = []
    hs_pre = bool(scratch and rows and P >= ENC_HS_PRE_MIN_POINTS)
    dh_hs = hs_pre and spec.Ls == spec.Ld
    pok = pair_ok(spec, table_aligned16)
    n_chunks = 0
    if scratch:
        assert max(spec.hd[1].size[-1], spec.hd[2].size[-1]) <= DH_MAX_ENTRIES
        n_chunks = min(256, max(1, ceil_div(P, 8192)))
        n_chunks = ceil_div(P, ceil_div(P, n_chunks))
        k += ["warp_coords", "dynhash_hs_fwd_lds<pair>" if dh_hs and pok else "dynhash_hs_fwd_lds<nopair>" if dh_hs else "dynhash_fwd_lds"]
    if hs_pre and not dh_hs:
        k.append("hashgrid_levels_launch")
    if rows:
        k.append("plane_time_rows")
    fused = bool(sigma and hs_pre and sigma == (128, 1))
    if fused:
        k.append("encode<hdt,rows,hs=1,sigma>")
    elif hs_pre:
        k.append("encode<hdt,rows,hs=1>")
    elif scratch and rows:
        k.append("encode<hdt,rows,hs=2>" if pok else "encode<hdt,rows,hs=0>")
    else:
        k.append("encode<%s,%s,hs=0>" % ("hdt" if scratch else "-", "rows" if rows else "-"))
    if sigma and not fused:
        k.append("mlp_fwd_sigma")
    return dict(kernels=k, n_chunks=n_chunks, hs_pre=hs_pre, dh_hs=dh_hs, pair=pok)


def bwd_routes(spec, P, rows, gd_absmax, samples_per_ray, in_pad):
    """l4d_density_encode_bwd (field_bwd.hip): prep route, chunking, band list, hash task list."""
    if P == 0:
        return dict(kernels=[])
    L3, colD = spec.L3, spec.colD
    fused_prep = bool(gd_absmax and rows and colD % 8 == 0 and L3 % 8 == 0 and L3 <= 48 and in_pad % 8 == 0)
    staged = int(colD % 8 == 0 and L3 % 8 == 0)
    k = ["bs_scatter"]
    if not fused_prep:
        k.append("prep<staged>" if staged else "prep<unstaged>")
    n_chunks = min(256, max(1, ceil_div(P, 2048)))
    chunk = ceil_div(P, n_chunks)
    n_chunks = ceil_div(P, chunk)
    wave_skip = int(samples_per_ray > 0 and samples_per_ray % 64 == 0 and chunk % 64 == 0)

    def chunks_for(n):
        n = min(n, max(1, ceil_div(P, 32768)))
        c = ceil_div(ceil_div(P, n), 64) * 64
        return c, ceil_div(P, c)
    chunk_ps, n_chunks_ps = chunks_for(128) if wave_skip else (chunk, n_chunks)
    if rows:
        k.append("plane_time_rows")
        k.append("planes_dyn_wide" if fused_prep and L3 > 24 else "planes_dyn<rows,prep>" if fused_prep else "planes_dyn<rows,->")
    else:
        k.append("planes_dyn<-,->")
    bands = []
    for s in range(spec.n_scales):
        for j, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
            W, H = spec.plane_res[s][a], spec.plane_res[s][b]
            nrows = min(max(1, 65536 // (W * 32)), H)
            bands += [(s, j, r0, min(nrows, H - r0)) for r0 in range(0, H, nrows)]
    k.append("planes_static")
    tasks = []
    for group in (0, 1):
        max_entries, fit = (8192, 8192) if group == 0 else (16384, 8192)
        for p, g in enumerate(spec.hd):
            for lvl in range(g.n_levels):
                size = g.size[lvl]
                if (size <= fit) != (group == 0):
                    continue
                pow2 = size & (size - 1) == 0
                if size == 2 * max_entries and pow2 and g.hashed[lvl]:
                    tasks += [(p, lvl, "parity", size // 2)] * 2
                    continue
                form = "fast" if g.hashed[lvl] and pow2 else "generic"
                for lo in range(0, size, max_entries):
                    tasks.append((p, lvl, form + ("-range" if size > max_entries else ""), min(max_entries, size - lo)))
    k += ["dynhash_lds", "dynhash_expand"]
    return dict(kernels=k, fused_prep=fused_prep, staged=staged, wide=bool(fused_prep and L3 > 24), n_chunks=n_chunks, chunk=chunk,
                wave_skip=wave_skip, chunk_ps=chunk_ps, n_chunks_ps=n_chunks_ps, bands=bands, tasks=tasks,
                task_forms=sorted({t[2] for t in tasks}), dense_levels=sorted({(t[0], t[1]) for t in tasks if t[2].startswith("generic")}))


# ---- the cases both test files walk --------------------------------------------------------------------------------------------------
def fwd_combo_cases(scratch):
    """(P, (frame, num_frames), in_pad) of test_forward_rows_every_pointer_combination."""
    pts = FWD_POINTS_SCRATCH if scratch else FWD_POINTS
    return [(P, FRAMES[i % len(FRAMES)], (96, 128, 192)[i % 3]) for i, P in enumerate(pts)] + [(257, fr, 128) for fr in FRAMES]


def bwd_args(i):
    """Frame and param_scale of the i-th point count."""
    return FRAMES[i % len(FRAMES)], PARAM_SCALES[i % 2]


FWD_PAIR_CASES = ((65, (25, 51)), (4159, (22, 51)))
FWD_OTHER = ((4, 64), (16, 192), ("6/8", 96))
FWD_OTHER_CASES = ((4159, False, False), (4159, True, True), (65, True, False), (65, False, True))
BWD_OTHER_POINTS = (129, 1025, 4159)
BWD_OTHER_POINTERS = ((False, False), (True, False), (False, True))  # (plane_rows, gd_absmax)
BWD_RANGE_CASES = ((4159, (22, 51)), (1025, (0, 51)))
FWD_POINTS = (0, 1, 63, 64, 65, 257, 4159)
FWD_POINTS_SCRATCH = FWD_POINTS + (8193,)
FWD_BIG = ((1 << 18) - 1, 1 << 18, (1 << 18) + 77)
BWD_POINTS = (0, 1, 63, 64, 65, 127, 128, 129, 767, 768, 769, 1023, 1024, 1025, 2047, 2048, 2049, 4159)
BWD_PREP = ((4, 64), (8, 128), (16, 192))  # (spec, in_pad): un-staged prep, staged / fused prep, wide
BAND_RAYS = (32, 64, 35 * 32)  # x 64 samples = 2,048, 4,096 and 71,680 rows
PARAM_SCALES = (1.0, 2.0 ** -7)
FWD_BIG_CASES = ((8, True, FWD_BIG), (8, False, FWD_BIG[1:2]), ("6/8", True, FWD_BIG))  # (spec, static table 16-byte aligned, point counts)


@functools.lru_cache(maxsize=2)
def bwd_case(spec_name, P, frame, num_frames, in_pad, param_scale, key=0):
    """Lattice cloud: references, bounds and prefills for one adjoint call with samples_per_ray = 0 (``route``: the default pointers;
    chunk sizes and workgroup counts, which the bounds use, do not depend on the pointers)."""
    spec = SPECS[spec_name]
    params = params_of(spec)
    t, tinfo, tinfo8 = frame_info(frame, num_frames)
    xt, flow16 = cloud(P, t, key)
    dX = make_dX(spec, P, in_pad, key)
    route = bwd_routes(spec, P, True, True, 0, in_pad)
    g0_arena = hc.prefill(spec.plane_numel, param_scale, 301)
    g0_hs = hc.prefill(spec.hs.n_entries * 4, param_scale, 303)
    g0_hd = [[hc.prefill(g.n_entries * 4, 1.0, 305, p, s) for s in range(spec.n_slices)] for p, g in enumerate(spec.hd)]
    out = dict(spec=spec, params=params, tinfo=tinfo, tinfo8=tinfo8, xt=xt, flow16=flow16, dX=dX, route=route, g0_arena=g0_arena,
               g0_hs=g0_hs, g0_hd=g0_hd, P=P, in_pad=in_pad, param_scale=param_scale)
    if P == 0:
        return out
    arena, hs, hd, dflow = encode_adjoint_ref(spec, params, xt, flow16, tinfo, in_pad, dX, param_scale)
    pb = plane_adjoint_bounds(spec, params, xt, flow16, tinfo, dX, param_scale, route, g0_arena)
    hs_bits = to_f32_exact(hc.bwd_ref(spec.hs, np.ascontiguousarray(xt[:, :3]), np.asarray(dX[:, spec.colsA:spec.colD], F64), param_scale,
                                      g0=g0_hs), "static table gradient")
    assert np.allclose(hs_bits.astype(F64) - g0_hs.astype(F64), hs, rtol=0, atol=1e-9)
    hd_bits = slice_grads_expected(spec, xt, tinfo, dX, param_scale, g0_hd)
    for p in range(3):  # the class E values agree with the float64 adjoint
        for s in range(spec.n_slices):
            ref = g0_hd[p][s].astype(F64) + hd[p][s]
            assert np.abs(hd_bits[p][s].astype(F64) - ref).max() <= 4 * U * np.abs(ref).max() + 1e-30
    out.update(arena=arena + g0_arena.astype(F64), bound=pb["bound"], seen=pb["seen"], vmax=pb["vmax"], gd_max=pb["gd_max"],
               hs_bits=hs_bits, hd_bits=hd_bits, dflow=dflow, dflow_bound=dflow_bound(spec, params, xt, flow16, tinfo, dX, dflow))
    return out


@functools.lru_cache(maxsize=1)
def band_case(n_rays, frame=25, num_frames=51, in_pad=128, param_scale=2.0 ** -7):
    """Ray cloud with samples_per_ray = 64 (band skip on), rows and gd_absmax given (the default route).
    At 71,680 rows the worst-case bounds grow with the number of contributions per texel while a contribution does not: a time-plane
    row element of 64 x 7 texels receives 2,240 fixed-point adds of up to q / 2 = 3e-6 each, a 64 x 64 static texel 70 contributions
    with 2^-11 of their magnitudes; a lost contribution would hide in either.  That case therefore carries no time-plane gradient (the
    time-plane kernel is judged at up to 4,159 rows, one and two chunks) and a static-plane gradient in a tenth of its rows: what it
    is for, the band skip and the three ragged chunks of planes_static_lds_kernel and dynhash_lds_kernel, sees every row either way."""
    spec = SPECS[8]
    params = params_of(spec)
    t, tinfo, tinfo8 = frame_info(frame, num_frames)
    xt, flow16 = ray_cloud(n_rays, t)
    P = xt.shape[0]
    dX = make_dX(spec, P, in_pad, 5, sparse_planes=0.9 if n_rays > 64 else 0.0)
    dX[:, spec.colsA:spec.colD] = 0.0  # (the static grid's weights are no fp32 lattice here: no gradient, the table keeps its bits)
    route = bwd_routes(spec, P, True, True, 64, in_pad)
    g0_arena = hc.prefill(spec.plane_numel, param_scale, 311)
    g0_hs = hc.prefill(spec.hs.n_entries * 4, param_scale, 313)
    g0_hd = [[hc.prefill(g.n_entries * 4, 1.0, 315, p, s) for s in range(spec.n_slices)] for p, g in enumerate(spec.hd)]
    arena, hs, hd, dflow = encode_adjoint_ref(spec, params, xt, flow16, tinfo, in_pad, dX, param_scale)
    assert not hs.any()
    pb = plane_adjoint_bounds(spec, params, xt, flow16, tinfo, dX, param_scale, route, g0_arena)
    hd_ref = slice_grads_bound(spec, xt, tinfo, dX, param_scale, g0_hd, route["n_chunks_ps"])
    return dict(spec=spec, params=params, tinfo=tinfo, tinfo8=tinfo8, xt=xt, flow16=flow16, dX=dX, route=route, g0_arena=g0_arena,
                g0_hs=g0_hs, g0_hd=g0_hd, P=P, in_pad=in_pad, param_scale=param_scale, arena=arena + g0_arena.astype(F64),
                bound=pb["bound"], seen=pb["seen"], vmax=pb["vmax"], gd_max=pb["gd_max"], hd_ref=hd_ref, dflow=dflow,
                dflow_bound=dflow_bound(spec, params, xt, flow16, tinfo, dX, dflow))
