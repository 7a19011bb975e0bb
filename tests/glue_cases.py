"""Inputs and references for the operator-level tests of the small kernels between the fused operators (tests/test_glue_cpu.py,
tests/test_gpu_glue_ops.py): the scene-flow glue of csrc/glue.hip, the chamfer distance of csrc/chamfer.hip, the attribute and
density-activation glue of csrc/render.hip, and the inputs of the unequal-resolution hex-plane test.  numpy only: importable
without a device, and nothing here is computed by HIP code.

Three kinds of reference.

E, exact emulation.  The library is compiled without fma contraction and with IEEE division, so a kernel that only adds,
multiplies, divides and converts is re-evaluated here in numpy float32 / float16 in the order the .hip file writes.  Bit-equal.

L, lattice.  Inputs are multiples of a power of two chosen so that every term and every partial sum is exact in fp32 in any
order; atomics and block reductions then equal the float64 evaluation bit for bit.  As in tests/mlp_exact_ref.py the reference
ASSERTS this (``assert_lattice``: all terms multiples of the unit, sum of magnitudes below 2^24 units), so that a bad lattice
fails on the CPU.

X, expf inside.  The float64 result rounded to the output type.  A case is near a boundary when the float64 value lies within
EXP_ULPS = 8 fp32 ulps (relative 8 * 2^-24) of an fp16 rounding midpoint: there either neighbouring fp16 value is accepted,
everywhere else the bits must agree (``x_check``).  expf is documented at 1 ulp and at most two more roundings follow; an error
in a clamp, a scale or an argument is at least one fp16 ulp, 2^13 times larger.  The near-boundary cases may number at most
X_CAP = 0.2 % of a test's cases (re-checked by test_glue_cpu.py: 60 of the 63,488 finite inputs for the sigmoid, 36 for
exp * 2^k with the k of ``sigma_d_pow2``).

Largest distances observed on an MI355X, in fp32 ulps (printed by test_gpu_glue_ops.py).  For an fp32 output the distance from
the float64 value is seen directly.  For an fp16 output it can only be seen where the kernel's value differs from the rounded
float64 value: it is then the distance of the float64 value from the rounding midpoint that the kernel's value crossed.
    l4d_attr_scatter (sigmoid, fp16)            1.00   (60 near-boundary cases per channel)
    l4d_sigma_from_h (exp, fp32, direct)        0.78   (43,778 results in fp32's normal range)
    l4d_sigma_bwd, l4d_sigma_bwd_rows (fp16)    0.45   (36 near-boundary cases)
"""
import numpy as np

F32, F16, F64 = np.float32, np.float16, np.float64
EXP_ULPS = 8
X_CAP = 0.002
EXACT_SUM = float(1 << 24)
CHAMFER_START = F32(3.4e38)  # csrc/chamfer.hip: best_d before the first candidate


def rng_of(*key):
    s = 23
    for k in key:
        s = (s * 1000003 + int(k) + 977) % ((1 << 31) - 1)
    return np.random.RandomState(s)


# ---- bit patterns ---------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Element-wise: equal bit patterns, NaN == NaN whatever the payload.  a, b arrays of one float type."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))


def all_f16():
    """Every fp16 bit pattern, in pattern order: 63,488 finite values, +-inf, 2,046 NaNs."""
    return np.arange(65536, dtype=np.uint16).view(F16)


def assert_lattice(terms, unit, axis=None, what=""):
    """Every term a multiple of ``unit`` and, along ``axis``, sum |terms| < 2^24 units: no partial sum rounds in fp32, in any order."""
    t = np.asarray(terms, dtype=F64) / unit
    assert np.isfinite(t).all() and (t == np.rint(t)).all(), f"{what}: not on the lattice of {unit}"
    tot = np.abs(t).sum(axis=axis)
    assert (tot < EXACT_SUM).all(), f"{what}: {float(np.max(tot))} units, not below 2^24"


def to_f32_exact(a, what=""):
    a = np.asarray(a, dtype=F64)
    r = a.astype(F32)
    assert (r.astype(F64) == a).all(), f"{what}: not exact in fp32"
    return r


# ---- X class --------------------------------------------------------------------------------------------------------------------
def _f16_ext(bits):
    """Value of a non-negative fp16 pattern as float64, with 0x7c00 standing for 2^16 (so that the last midpoint is 65520)."""
    bits = np.asarray(bits, dtype=np.int64)
    v = bits.astype(np.uint16).view(F16).astype(F64)
    return np.where(bits >= 0x7C00, 65536.0, v)


def x_classify(v64):
    """v64: finite float64 values.  -> (want fp16 = round-to-nearest-even of v64, other fp16 = the value on the far side of the
    nearest rounding midpoint, near [bool] = v64 within EXP_ULPS fp32 ulps of that midpoint, dist = that distance in fp32 ulps)."""
    v = np.asarray(v64, dtype=F64)
    assert np.isfinite(v).all()
    with np.errstate(over="ignore"):
        want = v.astype(F16)
    a = np.abs(v)
    wb = (np.abs(want).view(np.uint16)).astype(np.int64)  # 0 .. 0x7c00, ordered like the magnitudes
    w = _f16_ext(wb)
    up = a >= w  # the nearest midpoint lies above the rounded magnitude
    ob = np.where(up, wb + 1, np.maximum(wb - 1, 0))
    mid = 0.5 * (w + _f16_ext(ob))
    ulp32 = np.maximum(a, 2.0 ** -126) * 2.0 ** -24
    dist = np.abs(a - mid) / ulp32
    near = (dist <= EXP_ULPS) & (ob != wb)
    sign = np.where(np.signbit(v), 0x8000, 0)
    other = (np.minimum(ob, 0x7C00) | sign).astype(np.uint16).view(F16)
    return want, other, near, dist


def x_check(got16, v64, what):
    """The X rule for an fp16 output.  -> (number of near-boundary cases, largest distance in fp32 ulps among the cases whose
    bits differ from fp16(v64), 0.0 if none).  Raises AssertionError where the rule is broken."""
    got16 = np.asarray(got16)
    assert got16.dtype == F16
    want, other, near, dist = x_classify(v64)
    eq = same_bits(got16, want)
    ok = eq | (near & same_bits(got16, other))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"{what}: {bad.size} of {ok.size} cases differ from fp16(float64), first at {bad[:5]}: got "
                           f"{got16.reshape(-1)[bad[:5]]}, want {want.reshape(-1)[bad[:5]]}, float64 {np.asarray(v64).reshape(-1)[bad[:5]]}")
    n_near = int(near.sum())
    assert n_near <= X_CAP * near.size, f"{what}: {n_near} near-boundary cases of {near.size}: the inputs do not test this kernel"
    return n_near, float(dist[~eq].max()) if (~eq).any() else 0.0


def sigmoid64(x):
    x = np.asarray(x, dtype=F64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def trunc_exp_bwd64(h0, d_sigma, loss_scale):
    """d_sigma * exp(clamp(h0, -15, 15)) * loss_scale in float64 (activation.py:6-20)."""
    return np.asarray(d_sigma, F64) * np.exp(np.clip(np.asarray(h0, F64), -15.0, 15.0)) * float(loss_scale)


def sigma_d_pow2(n):
    """d_sigma = +-2^k per row, k in -14 .. 3: with loss_scale = 128 and exp in [3.1e-7, 3.3e6] the products span fp16's
    subnormals to its overflow, and only expf rounds before the fp16 conversion."""
    i = np.arange(n)
    k = (i * 7 + i // 18) % 18 - 14
    return (np.where((i // 3) % 2 == 0, 1.0, -1.0) * np.exp2(k.astype(F64))).astype(F32)


SIGMA_SMALL_P = (1, 255, 257)


def sigma_small_case(P):
    """h0 [P] fp16 in (-20, 20) (both sides of the clamp at +-15) and d_sigma = +-2^k, for the launch shapes below and above one
    workgroup.  No case of these is near a boundary (asserted by test_glue_cpu.py), so every one must be bit-equal."""
    h0 = rng_of(53, P).uniform(-20.0, 20.0, size=P).astype(F16)
    return h0, sigma_d_pow2(P + 5)[5:]


# ---- scene-flow glue (csrc/glue.hip) --------------------------------------------------------------------------------------------
def flow_xt_ref(pc, t, bound):
    """E: [(pc + bound) / (2 bound), t]."""
    pc = np.asarray(pc, F32)
    b = F32(bound)
    den = F32(2.0) * b
    out = np.empty((pc.shape[0], 4), F32)
    out[:, :3] = (pc + b) / den
    out[:, 3] = F32(t)
    return out


def flow_warp_ref(pc, y16, variants):
    """E: out[v] = pc + fp32(float(y16[:, col0:col0+3]) * step): product rounded, then sum rounded."""
    pc = np.asarray(pc, F32)
    out = np.empty((len(variants), pc.shape[0], 3), F32)
    for v, (col0, step) in enumerate(variants):
        prod = y16[:, col0:col0 + 3].astype(F32) * F32(step)
        out[v] = pc + prod
    return out


def nn_ref(a, b):
    """Brute-force nearest neighbour of every a[i] in b, fp32, the expression order of chamfer_nn_kernel:
    d = (dx*dx + dy*dy) + dz*dz with dx = b - a; a candidate wins with a strict ``d < best`` from best = 3.4e38, index 0: the first
    minimum wins, a NaN distance never does, and a query no candidate beats keeps (3.4e38, 0).  -> dist [n] fp32, idx [n] int32."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    n = a.shape[0]
    dist, idx = np.empty(n, F32), np.empty(n, np.int32)
    for i0 in range(0, n, 512):
        q = a[i0:i0 + 512, None, :]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = b[None, :, 0] - q[:, :, 0], b[None, :, 1] - q[:, :, 1], b[None, :, 2] - q[:, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == F32
            d = np.where(d < CHAMFER_START, d, F32(np.inf))
        j = np.argmin(d, axis=1)  # first occurrence of the minimum
        dj = d[np.arange(d.shape[0]), j]
        none = np.isinf(dj)
        dist[i0:i0 + 512] = np.where(none, CHAMFER_START, dj)
        idx[i0:i0 + 512] = np.where(none, 0, j)
    return dist, idx


def chamfer_ref(xyz1, xyz2):
    """[b,n,3], [b,m,3] -> dist1 [b,n], dist2 [b,m], idx1, idx2 (``nn_ref`` both ways)."""
    r1 = [nn_ref(p, q) for p, q in zip(xyz1, xyz2)]
    r2 = [nn_ref(q, p) for p, q in zip(xyz1, xyz2)]
    return (np.stack([r[0] for r in r1]), np.stack([r[0] for r in r2]), np.stack([r[1] for r in r1]), np.stack([r[1] for r in r2]))


def seg_for(n, m, b):
    """csrc/chamfer.hip seg_for, restated: -> (number of candidate segments launched, their length)."""
    q_tiles = (n + 255) // 256
    segs = max(1, 2048 // max(1, q_tiles * b))
    segs = max(1, min(segs, (m + 1023) // 1024))
    seg_len = (m + segs - 1) // segs
    return (m + seg_len - 1) // seg_len, seg_len


def lattice_cloud(n, shift, key, lo=-1.0, hi=1.0):
    """[n,3] fp32 multiples of 2^-shift in [lo, hi)."""
    k = rng_of(3, n, shift, *key).randint(int(lo * (1 << shift)), int(hi * (1 << shift)), size=(n, 3))
    return (k.astype(F64) / (1 << shift)).astype(F32)


FLOW_GRAD_SHAPES = [(1, 1), (1, 300), (300, 1), (256, 256), (257, 255), (700, 300), (300, 700)]
FLOW_GRAD_TERMS = ((0.25, 0), (-2.0, 0), (-0.5, 3))  # (step, col0): forward + 1, forward + 2 into the same columns, then backward
FLOW_DY_UNIT = 2.0 ** -7  # coordinates on 2^-5, |step| >= 2^-2


def flow_grad_case(n, m, same_neighbour=False):
    """Three chamfer terms of one scene-flow loss on the 2^-5 lattice.  -> dict(dy0 [n,6] lattice sentinels, terms: list of
    dict(p, q, dist1, dist2, idx1, idx2, step, col0)) with dist / idx from ``nn_ref``.  same_neighbour: every q lies nearest to p[0]."""
    dy0 = (rng_of(5, n, m).randint(-64, 65, size=(n, 6)) * 8).astype(F64) * FLOW_DY_UNIT
    terms = []
    for v, (step, col0) in enumerate(FLOW_GRAD_TERMS):
        p, q = lattice_cloud(n, 5, (n, m, v, 0)), lattice_cloud(m, 5, (n, m, v, 1))
        if same_neighbour:  # p[0] at the centre of q's cube, every other p far outside
            q = lattice_cloud(m, 5, (n, m, v, 1), -0.25, 0.25)
            p = lattice_cloud(n, 5, (n, m, v, 0), 0.75, 1.0)
            p[0] = 0.0
        d1, i1 = nn_ref(p, q)
        d2, i2 = nn_ref(q, p)
        if same_neighbour:
            assert (i2 == 0).all()
        terms.append(dict(p=p, q=q, dist1=d1, dist2=d2, idx1=i1, idx2=i2, step=step, col0=col0))
    return dict(dy0=to_f32_exact(dy0), terms=terms)


def flow_chamfer_grad_ref(t, dy):
    """L: one l4d_flow_chamfer_grad launch in float64.  dy [n,6] float64 is updated in place; -> partial [ceil(max(n,m)/256)]."""
    p, q = t["p"].astype(F64), t["q"].astype(F64)
    n, m, step, c0 = p.shape[0], q.shape[0], float(t["step"]), t["col0"]
    d1 = ((p - q[t["idx1"]]) ** 2).sum(1)
    d2 = ((q - p[t["idx2"]]) ** 2).sum(1)
    assert (d1 == t["dist1"].astype(F64)).all() and (d2 == t["dist2"].astype(F64)).all(), "distances not exact on this lattice"
    g1 = step * (p - q[t["idx1"]])                 # into row k
    g2 = step * (p[t["idx2"]] - q)                 # into row idx2[j]
    mag = np.abs(dy[:, c0:c0 + 3]) + np.abs(g1)
    np.add.at(mag, t["idx2"], np.abs(g2))
    assert_lattice(np.concatenate([g1, g2]), FLOW_DY_UNIT, what="flow chamfer gradient")
    assert_lattice(mag, FLOW_DY_UNIT, axis=None, what="flow chamfer gradient sums")
    dy[:, c0:c0 + 3] += g1
    np.add.at(dy[:, c0:c0 + 3], t["idx2"], g2)
    blocks = (max(n, m) + 255) // 256
    part = np.zeros(blocks)
    for b in range(blocks):
        terms = np.concatenate([d1[b * 256:(b + 1) * 256], d2[b * 256:(b + 1) * 256]])
        assert_lattice(terms, 2.0 ** -10, what="flow chamfer partial")
        part[b] = terms.sum()
    return part


FINISH_PARTIALS = (0, 1, 1023, 1024, 1025, 3000)
FINISH_GROUND = (0, 1, 1024, 1500)
W_GROUND_LATTICE = 2.0 ** -10


def finish_case(n_partial, ng, n_dy, lattice=True):
    """-> dict(partial [n_partial] fp32, y_g [ng,16] fp16 or None, dy [n_dy] fp32).  lattice: integer partials whose total is 7,
    y_g multiples of 2^-8 below 2 with +0, -0 and both signs; otherwise positive real-valued partials and fp16 flows.
    Columns 6..15 of y_g are NaN."""
    r = rng_of(7, n_partial, ng, n_dy, lattice)
    if lattice:
        partial = r.randint(-8, 9, size=n_partial).astype(F64)
        if n_partial:
            partial[-1] += 7.0 - partial.sum()
        y = r.randint(-511, 512, size=(ng, 6)).astype(F64) / 256.0
    else:
        partial = r.uniform(0.0, 40.0, size=n_partial)
        y = r.uniform(-0.05, 0.05, size=(ng, 6))
    y_g = None
    if ng:
        y_g = np.full((ng, 16), np.nan, F16)
        y_g[:, :6] = y.astype(F16)
        flat = y_g[:, :6].reshape(-1)
        flat[1], flat[2] = F16(-0.75), F16(0.5)
        flat[0], flat[-1] = F16(0.0), F16(-0.0)
        if ng > 1:
            flat[5], flat[7] = F16(-0.0), F16(0.0)
        y_g[:, :6] = flat.reshape(ng, 6)
    dy = r.uniform(-3.0, 3.0, size=n_dy).astype(F32)
    if n_dy:
        dy[r.randint(n_dy)] = F32(-7.25)  # the maximum is a negative value
    return dict(partial=partial.astype(F32), y_g=y_g, dy=dy)


def flow_loss_finish_ref(c, w_ground, lattice=True):
    """-> (loss float64, dy_g [ng,6] fp32 or None, amax [2] fp32, bound): L on the lattice (bound 0); otherwise
    bound = len * 2^-24 * sum |terms|, which holds for the fp32 sum of the terms in any order."""
    w = float(F32(w_ground))
    partial = c["partial"].astype(F64)
    y = np.zeros((0, 6)) if c["y_g"] is None else c["y_g"][:, :6].astype(F64)
    ng = y.shape[0]
    loss = 0.5 * partial.sum() + w * np.abs(y).sum()
    bound = 0.0
    if lattice:
        assert_lattice(partial, 1.0, what="partials")
        assert_lattice(y, 2.0 ** -8, what="ground flow")
        assert_lattice([0.5 * partial.sum(), w * np.abs(y).sum()], w * 2.0 ** -8, what="loss")
    else:
        bound = (partial.size + y.size + 2) * 2.0 ** -24 * (0.5 * np.abs(partial).sum() + w * np.abs(y).sum())
    dy_g = (F32(w_ground) * np.sign(y).astype(F32)).astype(F32) if ng else None  # sign(+-0) = 0: +0 after the product
    dy = c["dy"]
    if dy.size and not np.isfinite(dy).all():
        a0 = F32(np.inf)
    else:
        a0 = F32(np.abs(dy).max()) if dy.size else F32(0.0)
    return loss, dy_g, np.array([a0, F32(w_ground) if ng else F32(0.0)], F32), bound


def dy16_ref(dy, g, k):
    """E: fp16(fp32(dy * fp32(2^k * g))) in columns 0..5, +0 in 6..15."""
    s = F32(2.0 ** k) * F32(g)
    out = np.zeros((dy.shape[0], 16), F16)
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, :6] = (np.asarray(dy, F32) * s).astype(F16)
    return out


def dy16_scales():
    """(amax, g, kind) for l4d_flow_dy16: amax * |g| exact powers of two, one fp32 step below and above them, both clamps, g = 0,
    g < 0.  kind: 'k' = k must put amax * |g| * 2^k into [2^11, 2^12); 'edge' = within 2 fp32 ulps of a power of two, either
    neighbouring k; 'clamp+' / 'clamp-' = k = +40 / -40."""
    out = []
    for e in (-20, -3, 0, 1, 11, 12, 17):
        p = F32(2.0 ** e)
        out += [(p, F32(1.0), "edge"), (np.nextafter(p, F32(0)), F32(1.0), "edge"), (np.nextafter(p, F32(np.inf)), F32(1.0), "edge")]
    out += [(F32(0.75), F32(-4.0), "k"), (F32(3.0), F32(2.0 ** -9), "k"), (F32(1.37), F32(-0.0071), "k"), (F32(1000.0), F32(65536.0), "k"),
            (F32(2.0), F32(0.5), "edge"), (F32(1e-35), F32(1.0), "clamp+"), (F32(1e20), F32(1.0), "clamp-"), (F32(1.0), F32(0.0), "clamp+"),
            (F32(5.0), F32(-0.0), "clamp+")]
    return out


def axpy_ref(y, x, a):
    """E: y += fp32(a * x) where x != 0; elsewhere y keeps its bits."""
    out = y.copy()
    nz = x != 0
    with np.errstate(invalid="ignore", over="ignore"):
        out[nz] = y[nz] + F32(a) * x[nz]
    return out


AXPY_SIZES = (0, 1, 255, 257, 8192 * 256 + 3)  # the last one wraps the grid stride of axpy_dev_kernel (8192 blocks of 256)


def axpy_case(n):
    r = rng_of(11, n)
    x = r.uniform(-2.0, 2.0, size=n).astype(F32)
    y = r.uniform(-2.0, 2.0, size=n).astype(F32)
    if n >= 255:
        x[r.rand(n) < 0.5] = 0.0  # the gradient buffers are sparse
        x[3], y[3] = 0.0, F32(np.nan)
        x[4], y[4] = -0.0, F32(-0.0)
        x[5], y[5] = 0.0, F32(-0.0)
        x[n - 1], y[n - 1] = 0.0, F32(np.nan)
        x[n - 2] = 1.5
    return y, x, F32(r.uniform(0.1, 3.0))


# ---- float64 composition of the scene-flow loss (CPU side) ----------------------------------------------------------------------
def nn64(a, b):
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    j = d.argmin(1)
    return d[np.arange(a.shape[0]), j], j


def flow_loss_pieces64(pc, y, others, y_g, w_ground=0.001):
    """The loss of trainer.flow_loss composed from the pieces the kernels compute, in float64: warp, nearest neighbour,
    0.5 (sum d1 + sum d2) per term with its gradient as l4d_flow_chamfer_grad forms it, w_ground * L1 of the ground flow.
    y [n,6], y_g [ng,6]; others [(q [m,3], step, col0)].  -> (loss, d loss / d y [n,6], d loss / d y_g [ng,6])."""
    loss, dy = 0.0, np.zeros_like(y)
    for q, step, c0 in others:
        p = pc + y[:, c0:c0 + 3] * step
        d1, i1 = nn64(p, q)
        d2, i2 = nn64(q, p)
        loss += 0.5 * (d1.sum() + d2.sum())
        dy[:, c0:c0 + 3] += step * (p - q[i1])
        np.add.at(dy[:, c0:c0 + 3], i2, step * (p[i2] - q))
    loss += w_ground * np.abs(y_g).sum()
    return loss, dy, w_ground * np.sign(y_g)


# ---- chamfer edges (csrc/chamfer.hip) -------------------------------------------------------------------------------------------
CHAMFER_SHAPES = [(1, 1, 1), (1, 1, 2049), (1, 2049, 1), (2, 255, 1024), (3, 257, 1025), (1, 300, 3000)]
CHAMFER_MULTI_SEGMENT = [(1, 1, 2049), (3, 257, 1025), (1, 300, 3000)]  # direction 1 has more than one candidate segment
PLANT_A, PLANT_B = F32(1.0 / 32.0), F32(-3.0 / 32.0)  # odd multiples of 2^-5: on no point of the 2^-4 lattice


def plant_indices(m):
    """Where the copies of one candidate go: two in one LDS tile of the middle of the cloud, one further back."""
    return [m // 2, m // 2 + 10, (5 * m) // 6] if m >= 12 else []


def chamfer_case(b, n, m):
    """Clouds on the 2^-4 lattice in [-1, 1)^3 (natural ties), with exact copies of one candidate planted at ``plant_indices``
    in both directions and queries 0 and 1 placed on / next to the planted value.  -> xyz1 [b,n,3], xyz2 [b,m,3] fp32."""
    xyz1 = np.stack([lattice_cloud(n, 4, (b, n, m, i, 1)) for i in range(b)])
    xyz2 = np.stack([lattice_cloud(m, 4, (b, n, m, i, 2)) for i in range(b)])
    for (qs, cs, val) in ((xyz1, xyz2, PLANT_A), (xyz2, xyz1, PLANT_B)):
        J = plant_indices(cs.shape[1])
        if not J:
            continue
        cs[:, J, :] = val
        qs[:, 0, :] = val
        if qs.shape[1] > 1:
            qs[:, 1, :] = val + F32(1.0 / 16.0)
    return xyz1, xyz2


def chamfer_bwd_ref(xyz1, xyz2, gd1, gd2, idx1, idx2, g1_0, g2_0):
    """L: l4d_chamfer_bwd in float64 on top of the prefilled gradients.  chamfer3D.cu:154-173: g = 2 grad_dist[i];
    grad_a[i] += g (a_i - b_j); grad_b[j] -= g (a_i - b_j)."""
    g1, g2 = g1_0.astype(F64), g2_0.astype(F64)
    m1, m2 = np.abs(g1), np.abs(g2)
    unit = 2.0 ** -8
    for bi in range(xyz1.shape[0]):
        for a, b, gd, idx, ga, gb, ma, mb in ((xyz1[bi], xyz2[bi], gd1[bi], idx1[bi], g1[bi], g2[bi], m1[bi], m2[bi]),
                                              (xyz2[bi], xyz1[bi], gd2[bi], idx2[bi], g2[bi], g1[bi], m2[bi], m1[bi])):
            v = (2.0 * gd.astype(F64))[:, None] * (a.astype(F64) - b.astype(F64)[idx])
            assert_lattice(v, unit, what="chamfer gradient")
            ga += v
            ma += np.abs(v)
            np.add.at(gb, idx, -v)
            np.add.at(mb, idx, np.abs(v))
    assert_lattice(m1, unit, axis=None, what="chamfer gradient sums")
    assert (m1 / unit < EXACT_SUM).all() and (m2 / unit < EXACT_SUM).all()
    return g1, g2


# ---- attribute glue (csrc/render.hip) -------------------------------------------------------------------------------------------
GATHER_WIDTHS = [(64, 15, 96), (72, 15, 96), (80, 15, 96), (66, 15, 96), (16, 3, 32), (0, 15, 16), (8, 0, 16)]  # (n_enc, n_geo, in_pad)
SENTINEL16 = F16(-77.0)


def work_list(P, cap, key):
    """``cap`` distinct sample indices out of P, unsorted."""
    return rng_of(13, P, cap, *key).permutation(P)[:cap].astype(np.int32)


def gather_case(n_enc, n_geo, in_pad, cap, T, with_idx):
    n_rays = 5
    P = max(n_rays * T, cap)
    n_rays = -(-P // T)
    r = rng_of(17, n_enc, n_geo, in_pad, cap, T)
    dir_enc = r.uniform(-1, 1, size=(n_rays, max(n_enc, 1))).astype(F16)[:, :n_enc].copy()
    h = r.uniform(-4, 4, size=(n_rays * T, 16)).astype(F16)
    h[:, 0] = np.nan  # the density column: never part of a gathered row
    idx = work_list(n_rays * T, cap, (n_enc, T)) if with_idx else None
    return dict(dir_enc=dir_enc, h=h, idx=idx, T=T, cap=cap, n_enc=n_enc, n_geo=n_geo, in_pad=in_pad)


def attr_gather_ref(c, count):
    """Rows j < min(count, cap): [dir_enc[idx[j] // T] | h[idx[j], 1 : 1 + n_geo] | 1.0 ...]; the others keep the sentinel."""
    cap, T = c["cap"], c["T"]
    M = cap if count is None else min(count, cap)
    out = np.full((cap, c["in_pad"]), SENTINEL16, F16)
    for j in range(M):
        p = j if c["idx"] is None else int(c["idx"][j])
        out[j, :c["n_enc"]] = c["dir_enc"][p // T]
        out[j, c["n_enc"]:c["n_enc"] + c["n_geo"]] = c["h"][p, 1:1 + c["n_geo"]]
        out[j, c["n_enc"] + c["n_geo"]:] = F16(1.0)
    return out


def attr_scatter_bwd_ref(d_attr, attr_compact, idx, loss_scale):
    """E: fp16(((d * s) * (1 - s)) * loss_scale) in column 0 of [cap,16] rows, +0 elsewhere; -> (dy_raydrop, dy_intensity)."""
    outs = []
    for c in (0, 1):
        d, s = d_attr[idx, c].astype(F32), attr_compact[:, c].astype(F32)
        out = np.zeros((idx.shape[0], 16), F16)
        with np.errstate(over="ignore", invalid="ignore"):
            out[:, 0] = (((d * s) * (F32(1.0) - s)) * F32(loss_scale)).astype(F16)
        outs.append(out)
    return outs


GATHER_BWD_ROWS = [(32, 16, 15, 0), (96, 64, 15, 0), (32, 16, 15, 1), (32, 16, 7, 0)]  # (in_pad, n_enc, n_geo, h_layout)
GATHER_BWD_GENERIC = [(96, 66, 15, 0), (24, 16, 7, 0)]


def gather_bwd_case(in_pad, n_enc, n_geo, cap, P):
    r = rng_of(19, in_pad, n_enc, n_geo, cap)
    dxa_r = r.uniform(-300, 300, size=(cap, in_pad)).astype(F16)
    dxa_i = r.uniform(-300, 300, size=(cap, in_pad)).astype(F16)
    c0 = n_enc  # the first column either layout reads
    dxa_r[0, c0:c0 + 4] = [60000.0, np.inf, 60000.0, -60000.0]
    dxa_i[0, c0:c0 + 4] = [60000.0, -np.inf, -60000.0, -60000.0]
    return dict(dxa_r=dxa_r, dxa_i=dxa_i, idx=work_list(P, cap, (in_pad, n_enc)), P=P)


def attr_gather_bwd_ref(c, in_pad, n_enc, n_geo, h_layout, rows_kernel, count=None):
    """E: dh[idx[j], 1 + k] = fp16(float(dxa_r[j, col]) + float(dxa_i[j, col])), col = n_enc + k (+ 1 with h_layout).  The row
    kernel writes the whole row (column 0 and columns above n_geo are +0); the generic one leaves them as they were (sentinel)."""
    cap = c["idx"].shape[0]
    M = cap if count is None else min(count, cap)
    dh = np.full((c["P"], 16), SENTINEL16, F16)
    for j in range(M):
        p = int(c["idx"][j])
        if rows_kernel:
            dh[p] = F16(0.0)
        col = n_enc + (1 if h_layout else 0)
        with np.errstate(over="ignore", invalid="ignore"):
            dh[p, 1:1 + n_geo] = (c["dxa_r"][j, col:col + n_geo].astype(F32) + c["dxa_i"][j, col:col + n_geo].astype(F32)).astype(F16)
    return dh


# ---- hex planes with unequal resolutions ----------------------------------------------------------------------------------------
PLANES_RES = (6, 10, 12, 5)
PLANES_MS = (1, 3)
PLANES_TEXEL_EPS = 1e-4


def planes_resolutions():
    return [[r * m for r in PLANES_RES[:3]] + [PLANES_RES[3]] for m in PLANES_MS]


def planes_xt(P=2049):
    """P points in [-0.05, 1.05]^4, then rows exactly at 0, at 1 (every combination per axis pair) and on texel centres of both scales."""
    x = rng_of(29, P).uniform(-0.05, 1.05, size=(P, 4)).astype(F32)
    rows = [[0, 0, 0, 0], [1, 1, 1, 1], [0, 1, 0, 1], [1, 0, 1, 0], [0, 0.5, 1, 0.25], [0.3, 1, 0.7, 0], [1, 0.2, 0, 1]]
    for res in planes_resolutions():
        for i in range(max(res)):
            rows.append([min(i, r - 1) / (r - 1) for r in res])
    return np.concatenate([x, np.asarray(rows, F32)]) if P > 1 else x


def planes_dxt_mask(xt):
    """Rows whose float64 un-normalised coordinate is farther than 1e-4 texel from an integer on every axis of every scale:
    d/dxt jumps at the integers and fp32 may fall on the other side."""
    ok = np.ones(xt.shape[0], bool)
    for res in planes_resolutions():
        p = xt.astype(F64) * (np.asarray(res, F64) - 1.0)
        ok &= (np.abs(p - np.rint(p)) > PLANES_TEXEL_EPS).all(1)
    return ok
