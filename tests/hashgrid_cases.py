"""Inputs and float64 references for the exact tests of the hash-grid kernels (csrc/hashgrid.hip, csrc/hashgrid_dev.h) and of the
sorted gradient scatter (csrc/binscatter.hip): tests/test_hashgrid_cpu.py, tests/test_gpu_hashgrid_exact.py.  numpy only: importable
without a device, and nothing here is computed by HIP code.  ``same_bits``, ``assert_lattice``, ``to_f32_exact`` and ``rng_of`` are
those of tests/glue_cases.py, whose classes L and E (lattice, exact emulation) are used here as they are described there.

THE LATTICE (class L).  Six levels, base resolution 3, per-level scale 2: the float32 scales are exactly 2, 5, 11, 23, 47, 95 and
the resolutions 3 .. 96 (``Geom`` states them literally; test_hashgrid_cpu.py compares it with lidar4d_amd.gridmeta.GridMeta).
Coordinates are multiples of 1/16 from -1/16 to 17/16, so fmaf(scale, x, 0.5) is exact, the fractions are multiples of 1/16 and
every corner weight is a multiple of W_UNIT = 2^-8 (2-D) or 2^-12 (3-D).  The two values outside [0, 1] give cell -1 (levels 2 ..)
and cell == resolution: the index arithmetic wraps in uint32, restated below with numpy uint32.
  forward    table values are integers in [-8, 8]: every term w * v and every partial sum is a multiple of W_UNIT below 2^24 units,
             exact in fp32 in any order, with or without fma.  The output is fp16(float64 value), bit for bit.
  backward   dout is a multiple of 1/4 in [-2, 2], grad_scale a power of two: contributions are multiples of
             W_UNIT / 4 * grad_scale, and ``bwd_ref`` asserts that no entry's magnitudes (prefill included) reach 2^24 units.
  time       slice features are exact and rounded to fp16 by the kernel; slice pair, blend, Lagrange basis, the 4-term sum and the
             hs * basis * w product of the expand kernel are class E: numpy float32 in the order hashgrid.hip / common.h write them.

THE SORTED SCATTER AGAINST FLOAT64 (class B).  The dense levels of bs_scatter are run-merged fp32 atomics of lattice values: bit-exact.
A BINNED level (hashed, power-of-two size, 2 .. 256 bins of 2^shift entries, shift = 11 for NV = 2 or 4 values per entry and 13 for
NV = 1) cannot be; what the code (binscatter.hip) does to one contribution c = wx * u, u = w_yz * g, |g| <= G:
  (1) the record payload is fp16: of u (pair record), of c' = u * (1 - fx') or u * fx' (the halves of a pair that straddles two bins),
      or of a merged run's total.  Relative 2^-11 of what it rounds in fp16's normal range, at most 2^-25 below it;
  (2) the x weight of a pair record travels as fxq = floor(fx * 32767 + 0.5), the product rounded to fp32 first (|.| <= 2^-10 at
      2^15), and comes back as fp32(fxq * fp32(1 / 32767)) (2^-23 absolute) and as fp32(1 - that) (2^-25):
      EPS_FX = (0.5 + 2^-10) / 32767 + 2^-23 + 2^-25 = 2^-15.98, ABSOLUTE in the weight, i.e. EPS_FX * |u| in the contribution.
      (A term relative to c, 2^-15 * sum |c_i|, would be no bound: the code gives EPS_FX * sum |u_i|, larger by 1 / wx, up to 16 on
      this lattice.)  The fp32 products s * v of pass 2 and u * fx' of pass 1: 2^-23 |c| together;
  (3) pass 2 adds floor(p * fxs + 0.5) into int64, fxs = 2^(30 - e) with 1.01 * gmax < 2^e: half a quantum per add,
      <= 0.505 * gmax * 2^-29 (1 + 2^-23), and gmax, the largest |record value| pass 1 saw, is at most 64 G (a merged run of 64
      lanes): <= G * 2^-23 per add, at most one add per contribution;
  (4) the sum leaves pass 2 as fp32((double) sum * (out_scale / fxs)): 2^-24 of the result.
With second-order terms kept ((1 + 2^-10) on (2)), per table element i with contributions c_k, k = 1 .. n_i:
  B_i = grad_scale * [ (2^-11 + 2^-23) sum |c_k| + (1 + 2^-10) EPS_FX sum |u_k| + n_i (G 2^-23 + 2^-25) ],  bound_i = B_i + 2^-24 (|ref_i| + B_i).
No margin on top.  The test means something where a lost, doubled or misplaced record is seen: test_hashgrid_cpu.py asserts that at
least 95 % of the non-zero contributions to binned levels exceed twice their element's bound (scattered cloud 98.0 - 100 %, run cloud
97.7 - 99.9 %).

Largest |error| / bound observed on an MI355X on the binned levels, over the three grids and both sizes (printed by
test_gpu_hashgrid_exact.py::test_sorted_scatter_against_float64):
    scattered cloud    0.05 - 0.80 (3-D, F = 8: 0.77 - 0.80)      run cloud    0.20 - 0.93      one cell (merged runs)    < 0.001
    two cells          0.001 - 0.004                               x fraction within 2^-16 of 1    0.15 - 0.52
"""
import functools

import numpy as np

from glue_cases import EXACT_SUM, F16, F32, F64, assert_lattice, rng_of, same_bits, to_f32_exact  # noqa: F401 (re-exported)

PRIME1, PRIME2 = np.uint32(2654435761), np.uint32(805459861)  # tiny-cuda-nn's coherent-prime hash: index = x ^ y p1 ^ z p2
SCALES = tuple(float(3 * 2 ** lvl - 1) for lvl in range(16))  # 2, 5, 11, 23, 47, 95 and on: the field tests take up to 16 levels
COORD_DEN = 16
POINT_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4159)
GRAD_SCALES = (1.0, 0.25, 128.0)
EPS_FX = (0.5 + 2.0 ** -10) / 32767.0 + 2.0 ** -23 + 2.0 ** -25


class Geom:
    """The lattice grid, stated literally: GridMeta(n_dims, n_levels, F, log2T, base_resolution=3, per_level_scale=2.0)."""

    def __init__(self, n_dims, n_features, log2T, n_levels=6):
        self.n_dims, self.n_features, self.n_levels, self.log2T = n_dims, n_features, n_levels, log2T
        self.scale = [float(s) for s in SCALES[:n_levels]]
        self.res = [int(s) + 1 for s in self.scale]
        dense = [(r ** n_dims + 7) // 8 * 8 for r in self.res]
        self.size = [min(n, 1 << log2T) for n in dense]
        self.hashed = [r ** n_dims > n for r, n in zip(self.res, self.size)]
        self.offset = [int(v) for v in np.concatenate([[0], np.cumsum(self.size)[:-1]])]
        self.n_entries = int(sum(self.size))
        self.n_output_dims = n_levels * n_features
        self.w_unit = 2.0 ** (-4 * n_dims)

    def grid_meta_args(self):
        return (self.n_dims, self.n_levels, self.n_features, self.log2T, 3, 2.0)

    def level_slice(self, lvl, width):
        return slice(self.offset[lvl] * width, (self.offset[lvl] + self.size[lvl]) * width)


def default_log2T(D):
    return 12 if D == 3 else 10


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def lattice_points(n, D, *key):
    k = rng_of(31, n, D, *key).randint(-1, COORD_DEN + 2, size=(n, D))
    return (k.astype(F64) / COORD_DEN).astype(F32)


FULL = 4159  # the largest point count of the lattice tests: a smaller cloud is its first rows, so that per-point references are shared


@functools.lru_cache(maxsize=None)
def _coords_full(P, D, key):
    x = lattice_points(P, D, key)
    plant = np.array([[0, 0, 0], [16, 16, 16], [-1, -1, -1], [17, 17, 17], [-1, 17, 0], [16, -1, 17], [0, 16, -1]], F64)[:, :D]
    x[:7] = (plant / COORD_DEN).astype(F32)
    x.setflags(write=False)
    return x


def coords(P, D, key=0):
    """[P, D] fp32 multiples of 1/16 in [-1/16, 17/16]: the first P rows of one cloud of FULL points (of P points beyond that).  From 7
    points on it holds rows at 0, at 1, at both outside values and mixed; a single point is the one at 0."""
    return _coords_full(max(P, FULL), D, key)[:P].copy()


def run_lengths(P, key=0):
    """Runs of 1 .. 70 rows that cover 0 .. P - 1: some end on the 64-lane and 256-thread edges, most cross them, the last ends at P - 1."""
    r = rng_of(37, P, key)
    head = [60, 4, 1, 70, 57, 64, 64, 3, 69, 2, 70, 70, 13, 1, 1, 66]
    out, n = [], 0
    while n < P:
        ln = head[len(out)] if len(out) < len(head) else int(r.randint(1, 71))
        ln = min(ln, P - n)
        out.append(ln)
        n += ln
    return out


def run_cloud(P, D, key=0):
    """Consecutive rows repeat one lattice point, in runs of ``run_lengths``; neighbouring runs differ."""
    lens = run_lengths(P, key)
    pts = lattice_points(len(lens), D, 41, key)
    for i in range(1, len(lens)):
        if (pts[i] == pts[i - 1]).all():
            pts[i, 0] = F32(0.5) if pts[i, 0] != F32(0.5) else F32(0.25)
    return np.repeat(pts, lens, axis=0)


def one_cell_cloud(P, D, point=(0.25, 0.75, 0.25)):
    """Every point the same: fractions are multiples of 1/4 on every level (0 on level 0), so that sums over thousands of rows stay exact."""
    return np.tile(np.asarray(point[:D], F32), (P, 1))


def two_cell_cloud(P, D, a=(0.25, 0.75, 0.25), b=(0.75, 0.25, 0.5)):
    """Rows alternate between two points: no two neighbouring lanes share a cell (pair records, no merged runs), and every table
    element that is touched receives P / 2 contributions."""
    x = np.tile(np.asarray(a[:D], F32), (P, 1))
    x[1::2] = np.asarray(b[:D], F32)
    return x


FX_LEVEL = 5  # the finest level, binned in every class B grid


def fx_near_one_cloud(P, D):
    """The first coordinate puts the x fraction on level FX_LEVEL into [1 - 2^-16, 1), in cells 0 .. 7: fx * 32767 rounds up to the
    largest value of the pair record's 15-bit weight field (why BS_FX_ONE is 32767, not 2^15).  The other coordinates are on the lattice
    and differ from row to row, so that no two neighbouring lanes share a cell (pair records)."""
    scale = SCALES[FX_LEVEL]
    xs = []
    for n in range(8):
        x = F32((n + 0.5 - 2.0 ** -17) / scale)
        for _ in range(8):  # the nearest fp32 whose fmaf lands in the window
            frac = float(F32(F64(x) * scale + 0.5)) - n
            if 1.0 - 2.0 ** -16 <= frac < 1.0:
                break
            x = np.nextafter(x, F32(2.0) if frac < 1.0 - 2.0 ** -16 else F32(0.0))
        assert 1.0 - 2.0 ** -16 <= frac < 1.0, (n, frac)
        xs.append(x)
    out = lattice_points(P, D, 89)
    out[:, 1:] = np.clip(out[:, 1:], 0.0, 1.0)
    out[:, 0] = np.asarray(xs, F32)[np.arange(P) % 8]
    return out


def table_values(n, *key):
    """Integers in [-8, 8] as fp16."""
    return rng_of(43, n, *key).randint(-8, 9, size=n).astype(F16)


def dout_values(P, width, key=0, zero_rows=False):
    """Multiples of 1/4 in [-2, 2] as float64.  zero_rows: a tenth of the rows, and the whole wavefront of rows 128 .. 191, are zero."""
    r = rng_of(47, P, width, key)
    d = r.randint(-8, 9, size=(P, width)).astype(F64) / 4.0
    if zero_rows:
        d[r.rand(P) < 0.1] = 0.0
        d[128:192] = 0.0
    return d


def int_grads(P, width, key=0):
    """Integers in +-{1, 2, 3, 4} as float64 (class B)."""
    r = rng_of(53, P, width, key)
    return (r.randint(1, 5, size=(P, width)) * np.where(r.rand(P, width) < 0.5, -1.0, 1.0)).astype(F64)


def prefill(n, grad_scale, *key):
    """Lattice values for a gradient buffer that is accumulated into: multiples of grad_scale / 16, |.| <= 4 grad_scale, none zero."""
    k = rng_of(59, n, *key).randint(1, 65, size=n) * np.where(rng_of(61, n, *key).rand(n) < 0.5, -1.0, 1.0)
    return to_f32_exact(k * (float(grad_scale) / 16.0), "prefill")


def place(x, width, cols):
    """[P, width] fp32, NaN everywhere but x[:, d] in column cols[d]."""
    out = np.full((x.shape[0], width), np.nan, F32)
    for d, c in enumerate(cols):
        out[:, c] = x[:, d]
    return out


# (name, row width, columns for D = 3, starts one float into its buffer); D = 2 takes the first two columns
COORD_LAYOUTS = (("dense", None, (0, 1, 2), False), ("row4", 4, (0, 1, 2), False), ("row4_misaligned", 4, (0, 1, 2), True), ("row5_permuted", 5, (3, 1, 0), False))


# ---- the grid, restated ---------------------------------------------------------------------------------------------------------
def level_corners(geom, lvl, x, exact=True):
    """-> idx [P, 2^D] int64 (level-local entry), w [P, 2^D] float64 corner weight, u [P, 2^D] float64 weight without its x factor.
    locate / corner / grid_index of hashgrid_dev.h in float64 and numpy uint32; asserts that fmaf(scale, x, 0.5) is exact in fp32.
    exact=False (coordinates off the lattice): the float64 value, itself exact (a 7-bit scale times 24 bits, plus 0.5, for |x| >= 2^-20),
    rounded once to fp32, which is what fmaf does; fraction and weights are then exact in float64, not in fp32."""
    D, size, res = geom.n_dims, geom.size[lvl], np.uint32(geom.res[lvl])
    pos = x.astype(F64) * geom.scale[lvl] + 0.5
    if exact:
        assert (pos.astype(F32).astype(F64) == pos).all(), "fmaf(scale, x, 0.5) not exact"
    else:
        assert ((x == 0) | (np.abs(x) >= 2.0 ** -20)).all() and np.abs(x).max() < 2.0
        pos = pos.astype(F32).astype(F64)
    fl = np.floor(pos)
    frac = pos - fl
    cell = fl.astype(np.int64).astype(np.uint32)  # (uint32_t)(int) floor: -1 wraps to 0xffffffff
    P = x.shape[0]
    idx, w, u = np.empty((P, 1 << D), np.int64), np.empty((P, 1 << D), F64), np.empty((P, 1 << D), F64)
    with np.errstate(over="ignore"):
        for k in range(1 << D):
            wk, uk, g = np.ones(P), np.ones(P), []
            for d in range(D):
                bit = (k >> d) & 1
                f = frac[:, d] if bit else 1.0 - frac[:, d]
                wk = wk * f
                if d > 0:
                    uk = uk * f
                g.append(cell[:, d] + np.uint32(bit))
            if geom.hashed[lvl]:
                i = g[0].copy()
                if D > 1:
                    i ^= g[1] * PRIME1
                if D > 2:
                    i ^= g[2] * PRIME2
            else:
                i, stride = np.zeros(P, np.uint32), np.uint32(1)
                for d in range(D):
                    if int(stride) <= size:
                        i = i + g[d] * stride
                        stride = np.uint32((int(stride) * int(res)) & 0xFFFFFFFF)
            assert i.dtype == np.uint32
            idx[:, k], w[:, k], u[:, k] = i.astype(np.int64) % size, wk, uk
    return idx, w, u


def fwd_ref(geom, x, table16):
    """-> (float64 [P, L * F] exact values, fp16 of them).  Asserts the lattice of every term."""
    P, F, L = x.shape[0], geom.n_features, geom.n_levels
    tab = table16.astype(F64).reshape(-1, F)
    out = np.zeros((P, L * F))
    for p0 in range(0, P, 1 << 16):
        xs = x[p0:p0 + (1 << 16)]
        for lvl in range(L):
            idx, w, _ = level_corners(geom, lvl, xs)
            terms = w[:, :, None] * tab[geom.offset[lvl] + idx]
            assert_lattice(terms, geom.w_unit, axis=1, what="forward terms")
            out[p0:p0 + xs.shape[0], lvl * F:(lvl + 1) * F] = terms.sum(1)
    return out, out.astype(F16)


def needs_rounding(v64):
    return float(np.mean(v64.astype(F16).astype(F64) != v64))


def scatter64(geom, x, g64, width, want_abs=False):
    """sum over points and corners of w * g64[:, lvl * width + j] into a flat [n_entries * width] float64 table.
    -> (sums, sums of magnitudes, contributions per element) -- magnitudes and counts only if want_abs."""
    n = geom.n_entries * width
    tot, mag, cnt = np.zeros(n), np.zeros(n), np.zeros(n)
    for lvl in range(geom.n_levels):
        idx, w, _ = level_corners(geom, lvl, x)
        e = (geom.offset[lvl] + idx)[:, :, None] * width + np.arange(width)[None, None, :]
        c = w[:, :, None] * g64[:, None, lvl * width:(lvl + 1) * width]
        tot += np.bincount(e.ravel(), weights=c.ravel(), minlength=n)
        if want_abs:
            mag += np.bincount(e.ravel(), weights=np.abs(c).ravel(), minlength=n)
            cnt += np.bincount(e.ravel(), weights=(c != 0).ravel().astype(F64), minlength=n)
    return tot, mag, cnt


def bwd_ref(geom, x, dout64, grad_scale, width=None, g0=None):
    """Table gradient in float64: g0 + sum w * dout * grad_scale, [n_entries * width] (width: F, or F / 4 for the time kernels' Hs).
    Asserts the lattice: multiples of w_unit / 4 * grad_scale, and per element sum of magnitudes (prefill included) < 2^24 units."""
    width = geom.n_features if width is None else width
    unit = geom.w_unit / 4.0 * float(grad_scale)
    assert (dout64 * 4.0 == np.rint(dout64 * 4.0)).all(), "dout not on the lattice of 1/4"
    tot, mag, _ = scatter64(geom, x, dout64 * float(grad_scale), width, want_abs=True)
    if g0 is not None:
        tot, mag = tot + g0.astype(F64), mag + np.abs(g0.astype(F64))
    assert (tot / unit == np.rint(tot / unit)).all(), "table gradient: not on the lattice"
    assert (mag / unit == np.rint(mag / unit)).all() and (mag / unit < EXACT_SUM).all(), \
        f"table gradient: {float(mag.max() / unit)} units in one element, not below 2^24"
    bwd_ref.largest_log2_units = max(getattr(bwd_ref, "largest_log2_units", 0.0), float(np.log2(max(mag.max() / unit, 1.0))))
    return tot


# ---- time-blended kernels (class E) ---------------------------------------------------------------------------------------------
def lagrange4_f32(t):
    """common.h lagrange4: for j, the product over m != j (ascending) of fp32((t - fp32(T[m])) / fp32(T[j] - T[m])), first factor as is."""
    T = [0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0]
    t = F32(t)
    c = np.empty(4, F32)
    with np.errstate(all="ignore"):
        for j in range(4):
            p = None
            for m in range(4):
                if m == j:
                    continue
                f = F32(F32(t - F32(T[m])) / F32(T[j] - T[m]))
                p = f if p is None else F32(p * f)
            c[j] = p
    return c


def slice_pair_f32(t, n_slices):
    """common.h slice_pair -> (i1, i2, w1, w2)."""
    idx = F32(F32(t) * F32(n_slices - 1))
    f, c = np.floor(idx), np.ceil(idx)
    if int(f) == int(c):
        return int(f), int(c), F32(1.0), F32(0.0)
    return int(f), int(c), F32(c - idx), F32(idx - f)


def t_fwd_ref(geom, x, tables16, t):
    """-> fp32 [P, L * F / 4], as hashgrid_t_fwd_kernel computes it: slice features fp16(exact), blend w1 * a + w2 * b, then
    r = 0; r += basis[b] * a[b * FO + j], every operation rounded to fp32.  The fp16 output is this converted once more."""
    F, L, FO = geom.n_features, geom.n_levels, geom.n_features // 4
    i1, i2, w1, w2 = slice_pair_f32(t, len(tables16))
    basis = lagrange4_f32(t)
    a = fwd_ref(geom, x, tables16[i1])[1].astype(F32)
    if i1 != i2:
        b = fwd_ref(geom, x, tables16[i2])[1].astype(F32)
        a = w1 * a + w2 * b
    assert a.dtype == F32
    a = a.reshape(-1, L, 4, FO)
    r = np.zeros((x.shape[0], L, FO), F32)
    for bb in range(4):
        r = r + basis[bb] * a[:, :, bb, :]
    assert r.dtype == F32
    return r.reshape(x.shape[0], L * FO)


def t_expand_ref(geom, hs32, t, grads0):
    """hashgrid_t_expand_kernel on top of grads0 (list of n_slices fp32 [n_entries * F]): g[f] += (hs[f % FO] * basis[f / FO]) * w for the
    one or two slices t selects, only in entries where some hs is non-zero; the other slices and entries keep their bits."""
    F, FO = geom.n_features, geom.n_features // 4
    i1, i2, w1, w2 = slice_pair_f32(t, len(grads0))
    basis = lagrange4_f32(t)
    hs = hs32.reshape(-1, FO)
    live = (hs != 0).any(1)
    f = np.arange(F)
    with np.errstate(all="ignore"):
        prod = hs[:, f % FO] * basis[f // FO][None, :]  # [n_entries, F] fp32
        assert prod.dtype == F32
        out = [g.copy() for g in grads0]
        for i, w in ((i1, w1), (i2, w2)) if i1 != i2 else ((i1, w1),):
            g = out[i].reshape(-1, F)
            g[live] = g[live] + prod[live] * w
    return out


# ---- sorted scatter (class B) ---------------------------------------------------------------------------------------------------
BS_LISTS, BS_THREADS, BS_MAX_BINS = 8, 512, 256


def bs_shift(NV):
    return 13 if NV == 1 else 11


def binned_levels(geom, NV):
    """binscatter.hip bs_binned: hashed, a power-of-two size, 2 .. 256 bins of 2^shift entries."""
    out = []
    for lvl in range(geom.n_levels):
        n = geom.size[lvl]
        nb = (n + (1 << bs_shift(NV)) - 1) >> bs_shift(NV)
        out.append(bool(geom.hashed[lvl] and n & (n - 1) == 0 and 1 < nb <= BS_MAX_BINS))
    return out


def list_capacity(geom, NV, lvl, P):
    """binscatter.hip bs_plan: records one of the 8 lists of a bin holds."""
    nb = geom.size[lvl] >> bs_shift(NV)
    mean = P * (1 << (geom.n_dims - 1)) / (nb * BS_LISTS)
    cap = (int(mean * 1.25 + 8.0 * np.sqrt(mean) + 64.0) + 31) // 32 * 32
    return min(cap, ((P << geom.n_dims) + 31) // 32 * 32)


def list_overflows(geom, NV, x):
    """Does some list of some binned level receive more pair records than it holds?  For a cloud without merged runs, where every
    lane emits 2^(D-1) pair records per level into the bin of the pair's first corner.  Tile i of 512 rows is walked by workgroup
    b with i = (b % 8) * (grid / 8) + b / 8 (common.h xcd_tile), which appends to list b % 8: with fewer than 8 tiles some lists stay
    empty, and the others take more than the share they were sized for."""
    P, shift = x.shape[0], bs_shift(NV)
    n_wg = (P + BS_THREADS - 1) // BS_THREADS
    wg = np.arange(P) // BS_THREADS // ((n_wg + 7) // 8)
    assert wg.max() < BS_LISTS
    for lvl, binned in enumerate(binned_levels(geom, NV)):
        if not binned:
            continue
        idx = level_corners(geom, lvl, x)[0][:, 0::2]  # corners 2q: the pair's first entry
        nb = geom.size[lvl] >> shift
        cnt = np.bincount(((idx >> shift) * BS_LISTS + wg[:, None]).ravel(), minlength=nb * BS_LISTS)
        if cnt.max() > list_capacity(geom, NV, lvl, P):
            return True
    return False


def pow2_unit(v, smallest):
    """Largest power of two <= 1 that divides every value (at least ``smallest``, which must)."""
    unit = 1.0
    while unit > smallest and not (v / unit == np.rint(v / unit)).all():
        unit /= 2.0
    assert (v / unit == np.rint(v / unit)).all()
    return unit


def scatter_bound_ref(geom, x, g64, grad_scale=1.0, exact=True):
    """Class B reference for Hs of l4d_hashgrid_t_bwd's sorted route, NV = F / 4 values per entry.
    -> dict(ref, bound [n_entries * NV] float64 (bound 0 on the levels that are not binned: bit-exact there), binned [L] bool,
    seen: share of the non-zero contributions to binned levels that exceed twice their element's bound)."""
    NV = geom.n_features // 4
    gs = float(grad_scale)
    assert (g64 == np.rint(g64)).all() and np.abs(g64).max() <= 4.0
    G = float(np.abs(g64).max())
    n = geom.n_entries * NV
    binned = binned_levels(geom, NV)
    ref, bound = np.zeros(n), np.zeros(n)
    seen, total = 0, 0
    for lvl in range(geom.n_levels):
        idx, w, u = level_corners(geom, lvl, x, exact)
        e = ((geom.offset[lvl] + idx)[:, :, None] * NV + np.arange(NV)[None, None, :]).ravel()
        gl = g64[:, None, lvl * NV:(lvl + 1) * NV]
        c, cu = (w[:, :, None] * gl).ravel(), (u[:, :, None] * gl).ravel()
        ref += np.bincount(e, weights=c * gs, minlength=n)
        sl = geom.level_slice(lvl, NV)
        if not binned[lvl]:
            mag = np.bincount(e, weights=np.abs(c), minlength=n)[sl]
            unit = pow2_unit(c, geom.w_unit)
            assert (mag / unit < EXACT_SUM).all(), f"dense level {lvl}: {float(mag.max() / unit)} units, not below 2^24"
            continue
        nz = c != 0
        B = ((2.0 ** -11 + 2.0 ** -23) * np.bincount(e, weights=np.abs(c), minlength=n)
             + (1.0 + 2.0 ** -10) * EPS_FX * np.bincount(e, weights=np.abs(cu) * nz, minlength=n)
             + np.bincount(e, weights=nz.astype(F64), minlength=n) * (G * 2.0 ** -23 + 2.0 ** -25)) * gs
        B = B + 2.0 ** -24 * (np.abs(ref) + B)
        bound[sl] = B[sl]
        seen += int((np.abs(c[nz]) * gs > 2.0 * B[e[nz]]).sum())
        total += int(nz.sum())
    return dict(ref=ref, bound=bound, binned=binned, seen=seen / max(total, 1))


@functools.lru_cache(maxsize=None)
def scatter_case(D, F, P, cloud):
    """Class B inputs and reference.  3-D: log2T = 12 (F = 8: two bins of 2048 on levels 3 .. 5) or 14 (F = 4: two bins of 8192 on levels
    4, 5); 2-D: log2T = 12, so that level 5 (4096 entries, F = 8: two bins) is binned -- with the 2^10 of the lattice tests no 2-D level is."""
    geom = Geom(D, F, {(3, 8): 12, (3, 4): 14, (2, 8): 12}[(D, F)])
    x = {"scattered": lambda: coords(P, D, 71), "runs": lambda: run_cloud(P, D, 73), "one_cell": lambda: one_cell_cloud(P, D),
         "two_cells": lambda: two_cell_cloud(P, D), "fx_near_one": lambda: fx_near_one_cloud(P, D)}[cloud]()
    g = int_grads(P, geom.n_levels * (F // 4), 79)
    if cloud == "runs":
        g[rng_of(83, P).rand(P) < 0.1] = 0.0
    if cloud == "fx_near_one":  # off the lattice: the other levels' weights would round in fp32, so they get no gradient
        g[:, :FX_LEVEL * (F // 4)] = 0.0
    r = scatter_bound_ref(geom, x, g, exact=cloud != "fx_near_one")
    r.update(geom=geom, x=x, g=g)
    return r


SCATTER_DF = ((3, 8), (3, 4), (2, 8))
SCATTER_P = (2048, 8192)
SCATTER_CLOUDS = ("scattered", "runs", "one_cell", "two_cells", "fx_near_one")


# ---- cases shared by the CPU and the GPU tests ------------------------------------------------------------------------------------
DF = ((2, 2), (2, 4), (2, 8), (3, 2), (3, 4), (3, 8))
DF_T = ((2, 4), (2, 8), (3, 4), (3, 8))
# (slices, t): weights 1 / 0 and 0.5 / 0.5; one slice, no blend; and weights that are no powers of two (0.8 / 0.2 as fp32 computes them)
T_SETUPS = ((5, 0.0), (5, 0.375), (5, 1.0), (1, 0.0), (1, 0.3), (1, 1.0), (5, 0.3))
LEVELS_MIN_POINTS = 1 << 18  # l4d_hashgrid_t_fwd_ws: level-major kernels from here on


@functools.lru_cache(maxsize=None)
def _fwd_full(D, F, n_levels, log2T):
    geom = Geom(D, F, log2T, n_levels)
    x, table = coords(FULL, D, 3), table_values(geom.n_entries * F, D, F, n_levels)
    v64, out16 = fwd_ref(geom, x, table)
    return dict(geom=geom, x=x, table=table, v64=v64, out16=out16)


def fwd_case(D, F, P, n_levels=6, log2T=None):
    """The first P points of one cloud (the forward is evaluated point by point)."""
    c = _fwd_full(D, F, n_levels, default_log2T(D) if log2T is None else log2T)
    return dict(c, x=c["x"][:P], v64=c["v64"][:P], out16=c["out16"][:P])


def cloud_of(kind, P, D):
    return {"scattered": lambda: coords(P, D, 5), "runs": lambda: run_cloud(P, D, 7),
            "one_cell": lambda: np.tile(np.asarray([5, 7, 9][:D], F32) / F32(COORD_DEN), (P, 1))}[kind]()


@functools.lru_cache(maxsize=None)
def bwd_case(D, F, P, kind="scattered", grad_scale=1.0, prefilled=False, log2T=None):
    """dout64 [P, L * F] on the lattice of 1/4 (exact in fp16 and in fp32); zero rows inside the runs of the run cloud."""
    geom = Geom(D, F, default_log2T(D) if log2T is None else log2T)
    x = cloud_of(kind, P, D)
    dout = dout_values(P, geom.n_levels * F, 11, zero_rows=kind == "runs")
    g0 = prefill(geom.n_entries * F, grad_scale, D, F) if prefilled else np.zeros(geom.n_entries * F, F32)
    ref = to_f32_exact(bwd_ref(geom, x, dout, grad_scale, g0=g0), "table gradient")
    return dict(geom=geom, x=x, dout=dout, g0=g0, ref=ref)


@functools.lru_cache(maxsize=None)
def _t_fwd_full(D, F, n_slices, t):
    geom = Geom(D, F, default_log2T(D))
    x = coords(FULL, D, 13)
    tables = [table_values(geom.n_entries * F, D, F, 17, s) for s in range(n_slices)]
    return dict(geom=geom, x=x, tables=tables, out32=t_fwd_ref(geom, x, tables, t))


def t_fwd_case(D, F, P, n_slices, t):
    c = _t_fwd_full(D, F, n_slices, t)
    return dict(c, x=c["x"][:P], out32=c["out32"][:P])


@functools.lru_cache(maxsize=None)
def hs_case(D, F, P, kind, grad_scale):
    """Hs [n_entries * F / 4] of the time kernels' adjoint: the exact sum of corner weight * dout * grad_scale."""
    geom = Geom(D, F, default_log2T(D))
    x = cloud_of(kind, P, D)
    dout = dout_values(P, geom.n_levels * (F // 4), 19, zero_rows=kind == "runs")
    return dict(geom=geom, x=x, dout=dout, hs=to_f32_exact(bwd_ref(geom, x, dout, grad_scale, width=F // 4), "Hs"))


@functools.lru_cache(maxsize=None)
def t_bwd_case(D, F, P, n_slices, t, kind="scattered", grad_scale=1.0):
    """Every slice gradient prefilled; -> grads_ref: what each slice holds afterwards (the slices t does not select: their prefill)."""
    c = hs_case(D, F, P, kind, grad_scale)
    grads0 = [prefill(c["geom"].n_entries * F, 1.0, D, F, s) for s in range(n_slices)]
    return dict(c, grads0=grads0, grads_ref=t_expand_ref(c["geom"], c["hs"], t, grads0))


def big_rows(P, n_distinct=4096):
    """Row index into a small cloud for the one large case: the reference is evaluated on n_distinct points only."""
    return ((np.arange(P, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(9)).astype(np.int64) % n_distinct


@functools.lru_cache(maxsize=None)
def t_fwd_big_case():
    """D = 3, F = 8, L = 4, five slices at t = 0.375 (two of them blended), 2^18 rows drawn from 4096 points."""
    geom = Geom(3, 8, 12, n_levels=4)
    small = coords(4096, 3, 23)
    tables = [table_values(geom.n_entries * 8, 29, s) for s in range(5)]
    rows = big_rows(LEVELS_MIN_POINTS)
    return dict(geom=geom, x=small[rows], tables=tables, t=0.375, out16=t_fwd_ref(geom, small, tables, 0.375).astype(F16)[rows])
