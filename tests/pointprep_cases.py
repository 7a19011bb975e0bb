"""Seeded inputs, references and check bodies for the edge tests of the point-cloud preparation kernels (csrc/pointprep.hip):
tests/test_pointprep_cases_cpu.py and tests/test_gpu_pointprep_edges.py.  numpy only: importable without a device, nothing here
is computed by HIP code.

Every check body (``check_*``) takes a ``run`` callable with the C entry point's arguments as numpy arrays, the outputs prefilled
by the body, and gets back what the buffers hold afterwards.  The device tests pass a ``run`` that goes through ``_prep_lib.call``
or ``lidar4d_amd.pointprep``; the CPU tests pass the restatement of tests/pointprep_ref.py (``run_*_ref``), so every body is shown
to pass on the reference before it is asked of a kernel.

1. Compaction.  Row i of a cloud is (10 + (i mod 32768) / 1024, (i div 32768) / 64, 0) where it is kept and (100, 0, 0) where it
   is dropped: kept rows are distinct and exact in fp32 (16 significant bits), their distance lies in [10, 42.01] and z = 0, far
   from every limit of the default predicate.
2. Range predicate.  ``boundary_table``: one fp32 point on every boundary of the nine inequalities with a neighbour on either side.
   On a face of the ego box or a z limit the neighbour is one ulp of that coordinate away.  On a distance limit one ulp of a
   coordinate need not move the fp32 distance (x = 3 - 2^-22, y = 4: x^2 + y^2 = 25 - 1.5 * 2^-20 rounds back to 25 or to a tie),
   which would make the float32 and the float64 verdict differ; there the neighbour is the NEAREST value of the coordinate whose
   fp32 distance differs from the limit (``_dist_neighbour``), and the axis points (5, 0, 0), (0, 50, 0), ... are added, where
   sqrt(x * x) == |x| in fp32 and the neighbour is one ulp away indeed.  The CPU test shows float32 mask == float64 mask.
3. k-nearest mean distance.  ``knn_case(name)`` -> (points, the 65 smallest squared distances of every point in float64, sorted);
   ``knn_want`` takes the mean of the first k roots.  That is pointprep_ref.knn_mean_distance(method="brute") with the partition
   shared between the k (the CPU test shows the two bit-equal, and equal to the kd-tree form within 1e-9).
4. Outlier statistics.  ``outlier_avg``: seeded values in [0.5, 1.5], about 1 % of them 10 (at least one from n = 100 on).
5. Planes.  ``plane_cloud`` is range_filter(make_cloud(16, 256, seed=2))[:1000]; ``plane_triples`` draws 513 triples of distinct
   rows, cycling through the row ranges [0, 63), [0, 257) and [0, 1000): a third of the hypotheses stay in range -- the SAME
   planes -- when the cloud is cut to its first 63 or 257 points, the others are rejected there as out of range.  Triples 0, 255
   and 300 repeat a row (rejected: the first and the last of chunk one, and one inside chunk two); 256 and 512 (the first of
   chunk two, the only one of chunk three) are redrawn until the reference accepts them.
"""
import functools

import numpy as np

import pointprep_ref as ref
from glue_cases import F32, F64, rng_of, same_bits  # noqa: F401

SENT = F32(-12345.0)
ISENT = np.int32(-7)
PC_THREADS = 1024      # points per workgroup of the two compaction kernels
DEFAULT_LIMITS = (1.0, 50.0, -2.5, 4.0)
CUSTOM_LIMITS = (5.0, 50.0, -2.5, 4.0)


# =================================================================================================================================
# 1. ordered compaction
# =================================================================================================================================
COMPACT_N = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 3073)
COMPACT_PATTERNS = ("all", "none", "first", "last", "lane_1023", "lane_0_of_64", "alternating", "random_half")
COMPACT_BIG = 1025 * PC_THREADS + 1     # 1026 workgroups: workgroup 1025 sums the counts in front of it in two trips
WRAP = 32768


def keep_pattern(n, pattern, seed=0):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == n - 1
    if pattern == "lane_1023":
        return i % PC_THREADS == PC_THREADS - 1
    if pattern == "lane_0_of_64":
        return i % 64 == 0
    if pattern == "alternating":
        return i % 2 == 0
    assert pattern == "random_half"
    return rng_of(41, n, seed).uniform(size=n) < 0.5


def compact_points(keep):
    """[n, 3] fp32 (module docstring, 1.)."""
    n = keep.size
    i = np.arange(n)
    pts = np.zeros((n, 3), F64)
    pts[:, 0] = 10.0 + (i % WRAP) / 1024.0
    pts[:, 1] = (i // WRAP) / 64.0
    pts[~keep] = (100.0, 0.0, 0.0)
    out = pts.astype(F32)
    assert (out.astype(F64) == pts).all() and pts[:, 1].max(initial=0.0) < 1.0
    return out


def run_range_ref(points, n, limits, out, out_index, count):
    """l4dp_range_filter restated with pointprep_ref.range_filter_mask in float32: writes what the kernels write."""
    if n:
        with np.errstate(all="ignore"):
            mask = ref.range_filter_mask(points[:n], limits[0], limits[1], (limits[2], limits[3]))
        m = int(mask.sum())
        out[:m] = points[:n][mask]
        if out_index is not None:
            out_index[:m] = np.flatnonzero(mask)
    else:
        m = 0
    count[0] = m
    return out, out_index, count, points.copy()


def check_range_filter(run, points, want_mask, limits=DEFAULT_LIMITS, with_index=True, what=""):
    """One call with ``out`` ([n + 1, 3]: a guard row), ``out_index`` and ``count`` prefilled: count == want_mask.sum(); the first
    count rows are points[want_mask] bit for bit and in order; out_index is flatnonzero(want_mask); everything behind count keeps
    the sentinel; the points keep their bits."""
    n = points.shape[0]
    assert points.dtype == F32 and want_mask.shape == (n,)
    out = np.full((n + 1, 3), SENT, F32)
    out_index = np.full(n + 1, ISENT, np.int32) if with_index else None
    count = np.array([ISENT], np.int32)
    got, got_index, got_count, pts_after = run(np.ascontiguousarray(points).copy(), n, limits, out, out_index, count)
    m = int(want_mask.sum())
    assert int(got_count[0]) == m, f"count {int(got_count[0])} != {m} ({what}, n={n})"
    bad = np.flatnonzero(~same_bits(got[:m], points[want_mask]).all(axis=1))
    assert bad.size == 0, f"{what} n={n}: {bad.size} of {m} rows differ, first at output rows {bad[:4]}: {got[bad[:4]]}"
    assert same_bits(got[m:], np.full((n + 1 - m, 3), SENT, F32)).all(), f"{what} n={n}: rows behind count were written"
    if with_index:
        assert np.array_equal(got_index[:m], np.flatnonzero(want_mask)), f"{what} n={n}: out_index"
        assert (got_index[m:] == ISENT).all(), f"{what} n={n}: out_index behind count was written"
    assert same_bits(pts_after, points).all(), "the points were written"
    return got[:m]


def check_compaction(run, n, pattern, seed=0):
    keep = keep_pattern(n, pattern, seed)
    pts = compact_points(keep)
    for with_index in (True, False):
        check_range_filter(run, pts, keep, DEFAULT_LIMITS, with_index, what=f"pattern {pattern}")
    return int(keep.sum())


# =================================================================================================================================
# 2. the range predicate at its boundaries
# =================================================================================================================================
def _ulp_pair(v):
    v = F32(v)
    return np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))


def _dist32(p):
    p = np.asarray(p, F32)
    return np.sqrt(np.sum(p ** 2))


def _dist_neighbour(p, axis, direction):
    """The nearest fp32 value of coordinate ``axis`` in ``direction`` (+1: away from zero, -1: towards it) whose fp32 distance
    differs from that of p."""
    p = np.array(p, F32)
    d0 = _dist32(p)
    q = p.copy()
    toward = F32(np.inf) * np.sign(p[axis]) if direction > 0 else F32(0.0)
    for _ in range(16):
        q[axis] = np.nextafter(q[axis], toward)
        if _dist32(q) != d0:
            return q
    raise AssertionError("no neighbour within 16 ulp")


def boundary_table():
    """-> list of (name, limits, point [3] fp32).  Names end in '=' (on the boundary), '-' or '+' (the neighbour towards -inf /
    +inf of the coordinate, or for distances: towards / away from the origin)."""
    rows = []

    def add(name, limits, p):
        rows.append((name, limits, np.array(p, F32)))

    # distance limits (custom limits: dist_min = 5 lies outside the ego box)
    for name, p, axis in (("dist_min (3,4,0)", (3, 4, 0), 0), ("dist_min (3,4,0) y", (3, 4, 0), 1), ("dist_max (30,40,0)", (30, 40, 0), 0),
                          ("dist_max (30,40,0) y", (30, 40, 0), 1), ("dist_min (-3,-4,0)", (-3, -4, 0), 1),
                          ("dist_min (5,0,0)", (5, 0, 0), 0), ("dist_min (0,-5,0)", (0, -5, 0), 1),
                          ("dist_max (50,0,0)", (50, 0, 0), 0), ("dist_max (0,50,0)", (0, 50, 0), 1), ("dist_max (-50,0,0)", (-50, 0, 0), 0)):
        add(name + " =", CUSTOM_LIMITS, p)
        add(name + " -", CUSTOM_LIMITS, _dist_neighbour(p, axis, -1))
        add(name + " +", CUSTOM_LIMITS, _dist_neighbour(p, axis, +1))
    # the same distance points under the default limits: dist_min = 1 on an axis lies inside the ego box in x, outside it in y and z
    for name, p, axis in (("dist_min=1 (0,1,0)", (0, 1, 0), 1), ("dist_min=1 (0,-1,0)", (0, -1, 0), 1), ("dist_min=1 (1,0,0) in ego", (1, 0, 0), 0)):
        add(name + " =", DEFAULT_LIMITS, p)
        add(name + " -", DEFAULT_LIMITS, _dist_neighbour(p, axis, -1))
        add(name + " +", DEFAULT_LIMITS, _dist_neighbour(p, axis, +1))
    # z limits: x, y pass everything else
    for name, z in (("z_min", -2.5), ("z_max", 4.0)):
        lo, hi = _ulp_pair(z)
        for limits in (DEFAULT_LIMITS, CUSTOM_LIMITS):
            add(f"{name} =", limits, (10, 0, z))
            add(f"{name} -", limits, (10, 0, lo))
            add(f"{name} +", limits, (10, 0, hi))
    # the six faces of the ego box, each alone: the other two coordinates strictly inside, |p| > 1
    for name, axis, v, base in (("ego x=2", 0, 2.0, (0, 0.5, 0.5)), ("ego x=-2", 0, -2.0, (0, 0.5, 0.5)), ("ego y=1", 1, 1.0, (1, 0, 0.5)),
                                ("ego y=-1", 1, -1.0, (1, 0, 0.5)), ("ego z=2", 2, 2.0, (1, 0.5, 0)), ("ego z=-2", 2, -2.0, (1, 0.5, 0))):
        lo, hi = _ulp_pair(v)
        for tag, c in (("=", v), ("-", lo), ("+", hi)):
            p = list(base)
            p[axis] = c
            add(f"{name} {tag}", DEFAULT_LIMITS, p)
    # interior of the ego box (|p| > 1: only the box drops it), corners, non-finite coordinates
    add("ego interior", DEFAULT_LIMITS, (1.5, 0.5, 1.0))
    add("ego interior, negative", DEFAULT_LIMITS, (-1.5, -0.5, -1.0))
    add("ego corner", DEFAULT_LIMITS, (2, 1, 2))
    add("ego corner, negative", DEFAULT_LIMITS, (-2, -1, -2))
    add("kept", DEFAULT_LIMITS, (10, 10, 1))
    for axis in range(3):
        for name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            p = [10.0, 10.0, 1.0]
            p[axis] = v
            add(f"{name} in {'xyz'[axis]}", DEFAULT_LIMITS, p)
            add(f"{name} in {'xyz'[axis]}", CUSTOM_LIMITS, p)
    return rows


def boundary_clouds():
    """-> [(limits, names, points [m, 3] fp32, expected mask = pointprep_ref.range_filter_mask in float32)], one per limits."""
    out = []
    table = boundary_table()
    for limits in (CUSTOM_LIMITS, DEFAULT_LIMITS):
        names = [n for n, l, _ in table if l == limits]
        pts = np.stack([p for _, l, p in table if l == limits]).astype(F32)
        with np.errstate(all="ignore"):
            mask = ref.range_filter_mask(pts, limits[0], limits[1], (limits[2], limits[3]))
        out.append((limits, names, pts, mask))
    return out


def range_mask64(pts, limits):
    with np.errstate(all="ignore"):
        return ref.range_filter_mask(pts.astype(F64), limits[0], limits[1], (limits[2], limits[3]))


def check_boundaries(run):
    """Every point of the table alone (n = 1) and the whole table in one call, in table order and reversed."""
    kept = 0
    for limits, names, pts, mask in boundary_clouds():
        for i, name in enumerate(names):
            check_range_filter(run, pts[i:i + 1], mask[i:i + 1], limits, what=f"boundary point '{name}' {pts[i]}")
        check_range_filter(run, pts, mask, limits, what="boundary table")
        check_range_filter(run, pts[::-1].copy(), mask[::-1].copy(), limits, what="boundary table reversed")
        kept += int(mask.sum())
    return kept


# =================================================================================================================================
# 3. k-nearest mean distance
# =================================================================================================================================
KNN_RTOL = 1e-5      # tests/test_gpu_pointprep.py: fp32 inputs on both sides, about 70 roundings of 2^-24 per value on the device
KNN_KS = (1, 2, 7, 63, 64)
KNN_REF_COLS = 65    # one more than the largest k: shows ties AT the k-th distance
KNN_PAD_N = (65, 127, 128, 129, 4095, 4096, 4097, 8193)
KNN_CASES = ("lattice", "lattice_shuffled", "interleaved", "far_point", "flat", "line_x", "line_diagonal", "identical_200",
             "copies_70x64") + tuple(f"pad_{n}" for n in KNN_PAD_N)
INTERLEAVED_HALF = 4500
FAR_ROW = 1500


def knn_ks(name):
    return (64,) if name.startswith("pad_") else KNN_KS


def knn_points(name):
    if name.startswith("pad_"):
        n = int(name[4:])
        return rng_of(51, n).uniform(-20.0, 20.0, size=(n, 3)).astype(F32)
    if name in ("lattice", "lattice_shuffled"):
        g = np.arange(17, dtype=F32)
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return pts[rng_of(52).permutation(len(pts))] if name == "lattice_shuffled" else pts
    if name == "interleaved":
        a = rng_of(53).uniform(-20.0, 20.0, size=(INTERLEAVED_HALF, 3)).astype(F32)
        return np.concatenate([a, a + np.array([0.001, 0.0, 0.0], F32)]).astype(F32)
    if name == "far_point":
        pts = rng_of(54).uniform(0.0, 1.0, size=(3000, 3)).astype(F32)
        return np.insert(pts, FAR_ROW, np.array([1e6, 0.0, 0.0], F32), axis=0)
    if name == "flat":
        pts = rng_of(55).uniform(-20.0, 20.0, size=(3000, 3)).astype(F32)
        pts[:, 2] = 0.0
        return pts
    if name == "line_x":
        pts = np.zeros((3000, 3), F32)
        pts[:, 0] = rng_of(56).uniform(-30.0, 30.0, size=3000)
        return pts
    if name == "line_diagonal":
        t = rng_of(57).uniform(-10.0, 10.0, size=3000)
        return (t[:, None] * np.array([1.0, 2.0, -0.5])[None] + np.array([3.0, -1.0, 0.25])[None]).astype(F32)
    if name == "identical_200":
        return np.tile(np.array([[1.25, -3.5, 0.75]], F32), (200, 1))
    assert name == "copies_70x64"
    base = rng_of(58).uniform(-20.0, 20.0, size=(70, 3)).astype(F32)
    return np.repeat(base, 64, axis=0)[rng_of(59).permutation(70 * 64)]


def knn_smallest_d2(points, cols=KNN_REF_COLS):
    """The min(cols, n) smallest squared distances of every point to the cloud (itself included), ascending, in float64: the
    expression of pointprep_ref.knn_mean_distance(method="brute")."""
    pts = np.asarray(points, dtype=F64)[:, :3]
    n = len(pts)
    c = min(cols, n)
    out = np.empty((n, c))
    for i0 in range(0, n, 256):
        diff = pts[i0:i0 + 256, None, :] - pts[None, :, :]
        out[i0:i0 + 256] = np.sort(np.partition((diff * diff).sum(-1), c - 1, axis=1)[:, :c], axis=1)
    return out


def knn_want(d2, k):
    k = min(int(k), d2.shape[1])
    return np.sqrt(np.ascontiguousarray(d2[:, :k])).mean(axis=1)


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """-> (points [n, 3] fp32, smallest squared distances [n, min(65, n)] float64); computed once, not to be written to."""
    pts = np.ascontiguousarray(knn_points(name))
    d2 = knn_smallest_d2(pts)
    pts.setflags(write=False)
    d2.setflags(write=False)
    return pts, d2


def run_knn_kdtree(points, k, sort):
    return ref.knn_mean_distance(points, k, method="kdtree")


def check_knn(run, name, rtol=KNN_RTOL, sorts=(True, False)):
    """Both visiting orders, every k of the case: within rtol of the float64 reference, exactly 0 where the reference is 0; the
    figure of every call is printed before it is asserted.  -> the largest relative error."""
    pts, d2 = knn_case(name)
    worst = 0.0
    for k in knn_ks(name):
        want = knn_want(d2, k)
        for sort in sorts:
            got = np.asarray(run(pts, k, sort))
            assert got.shape == want.shape, (got.shape, want.shape)
            got = got.astype(F64)
            zero = want == 0
            err = np.abs(got[~zero] - want[~zero]) / want[~zero]
            e = float(err.max()) if err.size else 0.0
            worst = max(worst, e)
            print(f"knn {name}: n={len(pts)} k={k} sort={sort}: largest relative error {e:.3e} (bound {rtol:.0e}), "
                  f"{np.count_nonzero(got[zero])} of {np.count_nonzero(zero)} zero references not exactly 0")
            assert (got[zero] == 0).all(), f"knn {name} k={k} sort={sort}: {np.count_nonzero(got[zero])} values not exactly 0"
            assert e <= rtol, (f"knn {name} k={k} sort={sort}: relative error {e:.3e} > {rtol:.0e} at row "
                               f"{np.flatnonzero(~zero)[int(err.argmax())]}")
    return worst


# =================================================================================================================================
# 4. outlier statistics and the threshold compaction
# =================================================================================================================================
OUTLIER_N = (2, 3, 1023, 1024, 1025, 5000)
STATS_RTOL = 1e-10   # summation order alone: n 2^-53 = 6e-13 at n = 5000; the margin is for the subtraction in sd
STD_RATIO = 3.0
EQUAL_VALUE = F32(0.1)   # not dyadic; n a stays exact in float64 (24 + 13 bits), so mu == a, sd == 0 and threshold == a exactly


def outlier_avg(n, seed=0):
    r = rng_of(61, n, seed)
    v = r.uniform(0.5, 1.5, size=n).astype(F32)
    v[r.uniform(size=n) < 0.01] = 10.0
    if n >= 100:
        v[n // 2] = 10.0
    return v


def stats64(avg):
    """(mu, sd, threshold) in numpy float64 on the float32 values."""
    a = np.asarray(avg, F32).astype(F64)
    mu = a.mean()
    with np.errstate(all="ignore"):
        sd = np.sqrt(((a - mu) ** 2).sum() / (len(a) - 1))
    return mu, sd, mu + STD_RATIO * sd


def run_outlier_ref(points, avg, n, std_ratio, out, out_index, count, stats):
    """l4dp_outlier_filter restated with pointprep_ref.outlier_threshold."""
    a = avg[:n].astype(F64)
    thr = ref.outlier_threshold(a, std_ratio)
    mu = a.mean()
    stats[:] = (mu, (thr - mu) / std_ratio, thr)
    keep = a < thr
    m = int(keep.sum())
    out[:m] = points[:n][keep]
    out_index[:m] = np.flatnonzero(keep)
    count[0] = m
    return out, out_index, count, stats


def _outlier_call(run, avg):
    n = avg.size
    pts = compact_points(np.ones(n, bool))
    out = np.full((n + 1, 3), SENT, F32)
    out_index = np.full(n + 1, ISENT, np.int32)
    count = np.array([ISENT], np.int32)
    stats = np.full(3, -1.0, F64)
    got, got_index, got_count, got_stats = run(pts.copy(), np.ascontiguousarray(avg, F32).copy(), n, STD_RATIO, out, out_index, count, stats)
    return pts, got, got_index, int(got_count[0]), got_stats


def _check_kept(pts, got, got_index, m, rows, what):
    n = pts.shape[0]
    assert m == rows.size, f"{what}: count {m} != {rows.size}"
    assert np.array_equal(got_index[:m], rows), f"{what}: kept rows"
    assert same_bits(got[:m], pts[rows]).all(), f"{what}: kept points"
    assert same_bits(got[m:], np.full((n + 1 - m, 3), SENT, F32)).all() and (got_index[m:] == ISENT).all(), f"{what}: written behind count"


def check_outlier_mixed(run, n):
    """-> relative errors of (mu, sd, threshold) against numpy float64."""
    avg = outlier_avg(n)
    pts, got, got_index, m, stats = _outlier_call(run, avg)
    want = np.array(stats64(avg))
    err = np.abs(stats - want) / np.abs(want)
    print(f"outlier statistics n={n}: relative error of mu {err[0]:.3e}, sd {err[1]:.3e}, threshold {err[2]:.3e} (bound {STATS_RTOL:.0e}), "
          f"kept {m} of {n}")
    assert (err <= STATS_RTOL).all(), f"n={n}: stats {stats} against {want}: relative errors {err}"
    _check_kept(pts, got, got_index, m, np.flatnonzero(avg.astype(F64) < want[2]), f"outlier filter n={n}")
    return err


def check_outlier_equal(run, n):
    """n >= 2 equal values a: stats == (a, 0, a) exactly and nothing is kept (strict <)."""
    pts, got, got_index, m, stats = _outlier_call(run, np.full(n, EQUAL_VALUE, F32))
    a = float(EQUAL_VALUE)
    assert stats[0] == a and stats[1] == 0.0 and stats[2] == a, f"n={n}: stats {stats.tolist()} != ({a!r}, 0, {a!r})"
    _check_kept(pts, got, got_index, m, np.zeros(0, np.int64), f"all values equal, n={n}")


def check_outlier_single(run):
    """n = 1: mu is the value, sd = sqrt(0 / 0) and the threshold are NaN, nothing is kept."""
    avg = np.array([0.75], F32)
    pts, got, got_index, m, stats = _outlier_call(run, avg)
    assert stats[0] == 0.75 and np.isnan(stats[1]) and np.isnan(stats[2]), f"n=1: stats {stats.tolist()}"
    keep_ref = avg.astype(F64) < ref.outlier_threshold(avg, STD_RATIO)
    assert not keep_ref.any()
    _check_kept(pts, got, got_index, m, np.flatnonzero(keep_ref), "n=1")


# =================================================================================================================================
# 5. planes
# =================================================================================================================================
THR = 0.15
PLANE_BAND = 1e-4    # tests/test_gpu_pointprep.py: ten times the fp32 error of a plane distance at 50 m range
Y_GAP = 3.0
N_TRIPLES = 513      # chunks of 256, 256 and 1 hypotheses
TRIPLE_COUNTS = (513, 300, 257)
PLANE_POINT_COUNTS = (1000, 257, 63, 1)
TRIPLE_RANGES = (63, 257, 1000)
FORCED_INVALID = (0, 255, 300)
FORCED_VALID = (256, 512)   # the first hypothesis of chunk two and the only one of chunk three
MASK_N = (1, 255, 256, 257, 1000)
MASK_PLANES = (1, 6, 7)


@functools.lru_cache(maxsize=None)
def plane_cloud():
    pts = np.ascontiguousarray(ref.range_filter(ref.make_cloud(16, 256, seed=2))[:1000])
    assert pts.shape == (1000, 3) and pts.dtype == F32
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def plane_triples():
    r = rng_of(71, 4)   # a seed at which no hypothesis has a point within PLANE_BAND of the threshold on the 63-point cloud
    tri = np.stack([r.choice(TRIPLE_RANGES[h % 3], size=3, replace=False) for h in range(N_TRIPLES)]).astype(np.int32)
    for h in FORCED_INVALID:
        tri[h, 2] = tri[h, 0]
    for h in FORCED_VALID:         # redrawn until the reference accepts it
        while ref.sample_model(plane_cloud(), list(tri[h])) is None:
            tri[h] = r.choice(TRIPLE_RANGES[h % 3], size=3, replace=False)
    tri.setflags(write=False)
    return tri


def score_ref(data, triples, threshold=THR, y_gap=Y_GAP):
    """pointprep_ref.score_batch, with the header's rule for a row outside [0, n): rejected, not read.
    -> (valid [H] int32, coeffs [H, 4] fp32, counts [H] int32)."""
    triples = np.asarray(triples).reshape(-1, 3)
    n = len(data)
    inside = ((triples >= 0) & (triples < n)).all(axis=1)
    H = len(triples)
    valid, counts, coeffs = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros((H, 4), F32)
    if inside.any():
        with np.errstate(all="ignore"):
            v, c, co = ref.score_batch(data, triples[inside].astype(np.int64), threshold, y_gap)
        valid[inside], counts[inside], coeffs[inside] = v, c, co
    return valid, coeffs, counts


def run_score_ref(points, triples, y_gap, threshold):
    return score_ref(points, triples, threshold, y_gap)


def counts64(data, coeffs, valid, threshold=THR, band=PLANE_BAND):
    """Per hypothesis: (points with float64 distance < threshold, points within ``band`` of the threshold); 0 where invalid."""
    d64 = np.asarray(data, F32).astype(F64)
    cnt, bnd = np.zeros(len(valid), np.int64), np.zeros(len(valid), np.int64)
    for h in np.flatnonzero(valid):
        d = ref.plane_distance(d64, coeffs[h].astype(F64))
        cnt[h], bnd[h] = np.count_nonzero(d < threshold), np.count_nonzero(np.abs(d - threshold) < band)
    return cnt, bnd


def check_plane_score(run, n_points, n_triples):
    """valid and coeffs equal pointprep_ref.score_batch bit for bit (zeros where rejected); counts within the band of the float64
    counts, 0 where rejected; a second launch gives the same counts.  -> (valid hypotheses, largest |count - count_f64|)."""
    data, tri = plane_cloud()[:n_points], plane_triples()[:n_triples]
    valid_ref, coeffs_ref, _ = score_ref(data, tri)
    valid, coeffs, counts = run(data.copy(), tri.copy(), Y_GAP, THR)
    what = f"{n_points} points, {n_triples} triples"
    assert np.array_equal(valid, valid_ref), f"{what}: valid differs at {np.flatnonzero(valid != valid_ref)[:8]}"
    assert coeffs.dtype == F32 and coeffs.tobytes() == coeffs_ref.tobytes(), f"{what}: coefficients"
    bad = np.flatnonzero((valid_ref == 0) & (counts != 0))
    assert bad.size == 0, f"{what}: rejected hypotheses {bad[:8]} have counts {counts[bad[:8]]}"
    c64, band = counts64(data, coeffs_ref, valid_ref)
    diff = np.abs(counts.astype(np.int64) - c64)
    print(f"plane scoring, {what}: {int(valid_ref.sum())} valid, largest |count - count_f64| = {int(diff.max(initial=0))}, "
          f"largest band {int(band.max(initial=0))}")
    over = np.flatnonzero(diff > band)
    assert over.size == 0, f"{what}: hypotheses {over[:8]}: counts {counts[over[:8]]}, float64 {c64[over[:8]]}, band {band[over[:8]]}"
    _, _, again = run(data.copy(), tri.copy(), Y_GAP, THR)
    assert np.array_equal(again, counts), f"{what}: a second launch gave other counts"
    return int(valid_ref.sum()), int(diff.max(initial=0))


# a 7-point cloud of small dyadic values: every product and sum of the fit and of the distance numerator is exact in fp32
REJECT_CLOUD = np.array([[1.0, 0.0, 0.5],      # 0
                         [2.0, 3.0, 1.5],      # 1: |y0 - y1| = 3 exactly
                         [4.0, 1.0, 0.25],     # 2
                         [2.0, 2.5, 1.5],      # 3: |y0 - y3| = 2.5
                         [2.0, 3.0, 0.5],      # 4: p4 - p0 has a zero z component
                         [3.0, 6.0, 2.5],      # 5 = p0 + 2 (p1 - p0): collinear with 0 and 1
                         [4.0, 1.0, 0.25]], F32)   # 6 = point 2 under another index
REJECT_TRIPLES = np.array([[0, 1, 2], [1, 0, 2], [0, 3, 2], [0, 1, 1], [0, 0, 1], [0, 1, 0], [2, 2, 2], [0, 4, 2], [0, 1, 5], [0, 1, 6],
                           [2, 6, 0], [5, 0, 2]], np.int32)
REJECT_VALID = np.array([1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1], np.int32)


def check_plane_rejection(run):
    """Expectations from pointprep_ref.sample_model; REJECT_VALID is what this module claims they are."""
    want = [ref.sample_model(REJECT_CLOUD, list(t)) for t in REJECT_TRIPLES]
    assert [int(w is not None) for w in want] == REJECT_VALID.tolist()
    assert want[9].tobytes() == want[0].tobytes()               # the duplicate point gives the same plane
    valid_ref, coeffs_ref, counts_ref = score_ref(REJECT_CLOUD, REJECT_TRIPLES)
    valid, coeffs, counts = run(REJECT_CLOUD.copy(), REJECT_TRIPLES.copy(), Y_GAP, THR)
    assert np.array_equal(valid, REJECT_VALID), f"valid {valid.tolist()} != {REJECT_VALID.tolist()}"
    assert coeffs.tobytes() == coeffs_ref.tobytes(), coeffs
    assert coeffs[9].tobytes() == coeffs[0].tobytes() and np.any(coeffs[0] != 0)
    c64, band = counts64(REJECT_CLOUD, coeffs_ref, valid_ref)
    assert band.sum() == 0 and np.array_equal(counts_ref, c64)    # exact inputs: nothing near the threshold
    assert np.array_equal(counts, c64), f"counts {counts.tolist()} != {c64.tolist()}"
    assert counts[0] >= 5                                      # points 0, 1, 2, 5 and 6 lie in the plane of triple 0
    # a y gap of 3 against y_gap = 3 is accepted (not <); nextafter(3) rejects it
    above = float(np.nextafter(F32(3.0), F32(4.0)))
    valid2, coeffs2, counts2 = run(REJECT_CLOUD.copy(), REJECT_TRIPLES[:2].copy(), above, THR)
    assert valid2.tolist() == [0, 0] and not coeffs2.any() and not counts2.any()


MASK_PREFILL = np.array([0, 1, 2, 0x80, 0xFE], np.uint8)


def mask_planes():
    """Coefficients [7, 4] of the first seven valid hypotheses of the 1000-point cloud, and their fp32 reference counts."""
    valid, coeffs, counts = score_ref(plane_cloud(), plane_triples())
    h = np.flatnonzero(valid)[:7]
    return coeffs[h], counts[h], h


def run_mask_ref(points, coeffs, threshold, mask):
    for co in np.asarray(coeffs, F32).reshape(-1, 4):
        with np.errstate(all="ignore"):
            mask[ref.plane_distance(points, co) < threshold] |= 1
    return mask


def check_plane_mask(run, run_score, n):
    """n_planes in {1, 6, 7} on the first n points: mask == prefill | OR of the single-plane masks (bits set before the call
    survive); a single-plane mask agrees with float64 outside the band, is the prefix of the 1000-point one, and at n = 1000 its
    sum is the hypothesis's count; n_planes = 0 leaves the mask untouched."""
    data = plane_cloud()[:n]
    coeffs, _, hyp = mask_planes()
    d64 = data.astype(F64)
    singles = []
    for j in range(7):
        m = run(data.copy(), coeffs[j:j + 1].copy(), THR, np.zeros(n, np.uint8))
        assert m.dtype == np.uint8 and set(np.unique(m).tolist()) <= {0, 1}
        d = ref.plane_distance(d64, coeffs[j].astype(F64))
        clear = np.abs(d - THR) >= PLANE_BAND
        assert np.array_equal(m.astype(bool)[clear], (d < THR)[clear]), f"single-plane mask {j}, n={n}"
        singles.append(m)
    if n == len(plane_cloud()):
        _, _, counts = run_score(data.copy(), plane_triples().copy(), Y_GAP, THR)
        for j in range(7):
            assert int(singles[j].sum()) == int(counts[hyp[j]]), f"plane {j}: mask sum {int(singles[j].sum())}, count {int(counts[hyp[j]])}"
    else:
        full = plane_cloud()
        for j in range(7):
            big = run(full.copy(), coeffs[j:j + 1].copy(), THR, np.zeros(len(full), np.uint8))
            assert np.array_equal(big[:n], singles[j]), f"plane {j}: the mask of {n} points is not the prefix of the full one"
    prefill = MASK_PREFILL[rng_of(72, n).randint(0, MASK_PREFILL.size, size=n)]
    for n_planes in MASK_PLANES:
        union = np.zeros(n, np.uint8)
        for j in range(n_planes):
            union |= singles[j]
        got = run(data.copy(), coeffs[:n_planes].copy(), THR, np.zeros(n, np.uint8))
        assert np.array_equal(got, union), f"n={n} n_planes={n_planes}: not the OR of the single-plane masks"
        got = run(data.copy(), coeffs[:n_planes].copy(), THR, prefill.copy())
        bad = np.flatnonzero(got != (prefill | union))
        assert bad.size == 0, (f"n={n} n_planes={n_planes}: {bad.size} mask bytes are not prefill | near, first {bad[:4]}: "
                               f"prefill {prefill[bad[:4]]}, near {union[bad[:4]]}, got {got[bad[:4]]}")
    got = run(data.copy(), coeffs[:0].copy(), THR, prefill.copy())
    assert np.array_equal(got, prefill), "n_planes = 0 wrote the mask"
