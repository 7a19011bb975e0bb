"""Inputs, references and check bodies for the edge tests of the range-image conversions (tests/test_convert_cpu.py,
tests/test_gpu_convert_edges.py): pano_count_kernel / pano_emit_kernel (l4d_pano_to_lidar) and pano_fill_kernel / lidar_bin_kernel /
lidar_unpack_kernel (l4d_lidar_to_pano) of csrc/convert.hip.  numpy only: importable without a device, nothing here is computed by
HIP code.

Every check body (``check_*``) takes a ``run`` callable with the C entry point's arguments as numpy arrays, the outputs prefilled
by the body, and gets back what every buffer holds afterwards.  The device tests pass a ``run`` that goes through ``ops.call``;
tests/test_convert_cpu.py passes the float32 restatements below (``pano_to_lidar_f32``, ``lidar_to_pano_f32``), first as they are
(every body passes) and then with a ``fault`` (the body fails): prefix_one_sweep, tie_highest, depth_le.

References.
* Structure (which pixels, which order, which winner): oracle/convert_ref.py, pinned bit for bit to the reference project by
  tests/golden/convert.npz.  The restatements here are shown equal to it on every cloud and image of this module.
* Coordinates of pano_to_lidar: ``pixel_dirs64``, the float64 evaluation of the same formulas, and the bound DIR_K 2^-24 |range|.

Derivation of DIR_K (u = 2^-24, the unit roundoff: one fp32 rounding is at most u relative, and at most half an ulp of the
result's binade absolute; pixel_dir of csrc/convert.hip, step by step).
  beta = -((float)i - W/2) / W * 2 * (float)pi.  The subtraction is exact (integers below 2^24, halves).  The quotient lies in
  [-0.5, 0.5]: half an ulp there is u / 4, which * 2 pi makes 1.57 u.  * 2 is exact.  (float)pi is 0.467 u relative above pi:
  1.47 u at |beta| = pi.  The product lies in [-pi, pi]: half an ulp is 2 u.  |d beta| <= 5.04 u (reached: see the measurement).
  alpha = (fov_up - (float)j / H * fov) / 180 * (float)pi.  In degrees: j / H rounds, (float)fov rounds, the product rounds
  (3 u fov), (float)fov_up rounds (u |fov_up|), the difference rounds (u A, A = the largest |alpha| of the image in degrees);
  then / 180 rounds, (float)pi, the product rounds (2.467 u A).  |d alpha| <= (pi / 180) (3 fov + |fov_up| + 3.467 A) u:
  2.95 u for K = (2, 26.9), 4.08 u for (10, 40), 2.95 u for (10, 30).
  sinf, cosf: 1 ulp each (HIP's documented accuracy), results in [-1, 1]: s = 1 u.
  dx = cos(alpha) cos(beta): |d| <= |d alpha| + |d beta| + 2 s, the product rounds (0.5 u), the product with the range rounds
  (u |range|).  dy alike; dz = sin(alpha) has less.
  DIR_K(K) = 5.04 + alpha_term(K) + 2 + 0.5 + 1:  11.49 for (2, 26.9), 12.62 for (10, 40), 11.49 for (10, 30); plus half the
  smallest subnormal for a range whose product underflows.
Measured (tests/test_convert_cpu.py prints it): the float32 restatement ``pixel_dirs_f32`` against float64 at unit range,
largest component error in units of u:
    64 x 2048 (2, 26.9)   3.58      3 x 5 (10, 40)   2.90      66 x 515 (10, 30)   4.42      1 x 1050629 (2, 26.9)   5.03
-- at most 0.44 DIR_K (the last one: column 0, beta = -pi, where the three beta terms add up): inside the bound with the factor
two to spare that the CPU test requires (2.28 at the least).
MI355X (tests/test_gpu_convert_edges.py prints it), the kernel's xyz against the float64 product in units of u |range|: 5.26 on
1 x 1050629 (random 90 %), at most 4.73 on the small images (3 x 683).

Unambiguous clouds (``cloud``): one point per pixel, built in float64 at the pixel's centre plus a uniform offset of up to a
quarter pixel in both angles (column 0: column offset >= 0, it sits on atan2's branch cut), rounded to fp32, shuffled.  Bin-edge
margin = distance of the fp32 point's float64 fractional pixel from the nearest bin edge, smallest over the cloud (printed by the
CPU test, which requires >= 0.2 px):
    1 x 1 (10, 40)  0.295    3 x 5 (10, 40)  0.258    8 x 16 (2, 26.9)  0.252    16 x 257 (2, 26.9)  0.250
    66 x 515 (10, 30)  0.250    64 x 2048 (2, 26.9)  0.250    32 x 4096 (2, 26.9)  0.250    (the last two: CPU only)
An fp32 evaluation of the projection is a few 1e-4 px from the float64 one at W = 4096, so every point has one pixel whatever
atan2f returns, and the image is pano[r, c] = sqrt_f32((x^2 + y^2) + z^2) bit for bit (no contraction, correctly rounded sqrtf).

Not tested on the device: l4d_lidar_to_pano refuses n >= 2^32 (the point index is the low word of the 64-bit key).  Read from the
code: the test ``n >= (1ll << 32)`` comes after the H W = 0 return and before the first launch, sets the error text
"l4d_lidar_to_pano: more than 2^32 points" and returns 1, so nothing is written.  A wrong refusal would read 64 GB out of bounds,
which is why no test calls it.
"""
import numpy as np

from glue_cases import F32, F64, rng_of, same_bits  # noqa: F401

U = 2.0 ** -24
THREADS = 1024                     # CV_THREADS: pixels per workgroup of the two pano kernels
SENT = F32(-12345.0)
HALF_SUBNORMAL = 2.0 ** -150
PI32 = F32(np.pi)
PI_REL = (float(PI32) - np.pi) / np.pi / U      # 0.467: (float)pi above pi, in units of u relative
KITTI, WIDE, MID = (2.0, 26.9), (10.0, 40.0), (10.0, 30.0)


def dir_k(K):
    """DIR_K of the module docstring for lidar_K = (fov_up, fov)."""
    fov_up, fov = float(K[0]), float(K[1])
    A = max(abs(fov_up), abs(fov_up - fov))
    beta_term = 2 * np.pi * 0.25 + np.pi * PI_REL + 2.0
    alpha_term = np.pi / 180.0 * (3.0 * abs(fov) + abs(fov_up) + (2.0 + PI_REL + 1.0) * A)
    return beta_term + alpha_term + 2.0 + 0.5 + 1.0


# =================================================================================================================================
# 1a. pano_to_lidar
# =================================================================================================================================
def pixel_dirs64(H, W, K, idx):
    """float64 directions [n, 3] of the flat pixel indices idx: utils/convert.py:112-123 in double."""
    idx = np.asarray(idx, dtype=np.int64)
    col, row = (idx % W).astype(F64), (idx // W).astype(F64)
    beta = -(col - W / 2) / W * 2 * np.pi
    alpha = (float(K[0]) - row / H * float(K[1])) / 180 * np.pi
    return np.stack([np.cos(alpha) * np.cos(beta), np.cos(alpha) * np.sin(beta), np.sin(alpha)], -1)


def pixel_dirs_f32(H, W, K, idx):
    """pixel_dir of csrc/convert.hip in numpy float32, operation by operation."""
    idx = np.asarray(idx, dtype=np.int64)
    i, j = (idx % W).astype(F32), (idx // W).astype(F32)
    beta = -(i - F32(W) / F32(2.0)) / F32(W) * F32(2.0) * PI32
    alpha = (F32(K[0]) - j / F32(H) * F32(K[1])) / F32(180.0) * PI32
    ca = np.cos(alpha)
    d = np.stack([ca * np.cos(beta), ca * np.sin(beta), np.sin(alpha)], -1)
    assert d.dtype == F32
    return d


PANO_FAULTS = (None, "prefix_one_sweep")


def pano_to_lidar_f32(pano, inten, H, W, K, points, count, fault=None):
    """l4d_pano_to_lidar restated: per-workgroup counts, each workgroup's base = the counts in front of it (summed in sweeps of
    1024), rank inside the workgroup.  Writes into ``points`` [rows, 4] and ``count`` [1] like the kernels: nothing else is touched.
    fault 'prefix_one_sweep': the base sums only the first 1024 workgroups' counts."""
    assert fault in PANO_FAULTS
    n = H * W
    if n == 0:
        count[0] = 0
        return
    flat = pano.reshape(-1)[:n]
    idx = np.flatnonzero(flat != 0)
    nblk = -(-n // THREADS)
    blk = idx // THREADS
    counts = np.bincount(blk, minlength=nblk)
    front = np.concatenate([[0], np.cumsum(counts)])          # front[b] = points of workgroups 0 .. b - 1
    b = np.arange(nblk)
    base = front[np.minimum(b, THREADS)] if fault == "prefix_one_sweep" else front[b]
    pos = base[blk] + (np.arange(idx.size) - front[blk])
    with np.errstate(all="ignore"):
        xyz = pixel_dirs_f32(H, W, K, idx) * flat[idx][:, None]
    points[pos, :3] = xyz
    points[pos, 3] = inten.reshape(-1)[idx] if inten is not None else F32(0.0)
    count[0] = base[-1] + counts[-1]


def run_pano_f32(fault=None):
    """A ``run`` for check_pano_to_lidar from the restatement."""
    def run(pano, inten, H, W, K, points, count):
        p, i = pano.copy(), None if inten is None else inten.copy()
        pano_to_lidar_f32(p, i, H, W, K, points, count, fault)
        return points, count, p, i
    return run


PANO_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1)
PANO_BIG = (1, 1024 * 1026 + 5)          # 1027 workgroups: the prefix loop of workgroups 1025 and 1026 runs a second sweep
PATTERNS = ("empty", "full", "first", "last", "lanes_0_63", "every_1024th", "full_gap_one", "random10", "random90")


def pano_shapes():
    """(H, W) for every count: 1 x n, n x 1 and a factorisation with a W that is no power of two where n has one."""
    odd = {63: (7, 9), 65: (5, 13), 1023: (33, 31), 1024: (64, 16), 1025: (41, 25), 2049: (3, 683)}
    out = []
    for n in PANO_COUNTS:
        out += [(1, n), (n, 1)] if n > 1 else [(1, 1)]
        if n in odd:
            out.append(odd[n])
    return out


def occupancy(n, pattern, seed=0):
    i = np.arange(n)
    if pattern == "empty":
        return np.zeros(n, bool)
    if pattern == "full":
        return np.ones(n, bool)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == n - 1
    if pattern == "lanes_0_63":
        return (i % 64 == 0) | (i % 64 == 63)
    if pattern == "every_1024th":
        return (i % THREADS == 0) | (i % THREADS == THREADS - 1)
    if pattern == "full_gap_one":
        return (i < THREADS) | (i == n - 1)
    p = {"random10": 0.1, "random90": 0.9}[pattern]
    return rng_of(5, n, int(p * 10), seed).uniform(size=n) < p


def pano_image(H, W, pattern, seed=0):
    """[H, W] fp32: ranges 2 .. 72 where the pattern is set, +0.0 elsewhere."""
    n = H * W
    r = rng_of(6, n, seed).uniform(2.0, 72.0, size=n).astype(F32)
    return np.where(occupancy(n, pattern, seed), r, F32(0.0)).reshape(H, W)


SPECIAL_RANGES = dict(neg_zero=F32(-0.0), negative=F32(-7.25), nan=F32(np.nan), inf=F32(np.inf),
                      subnormal=np.array([1], np.uint32).view(F32)[0], huge=F32(3e38))


def special_image(H, W):
    """A 10 % random image with every special range placed twice: -0.0 is dropped, the others are kept."""
    pano = pano_image(H, W, "random10", 3).reshape(-1)
    where = {}
    for k, (name, v) in enumerate(SPECIAL_RANGES.items()):
        for p in (3 + 5 * k, pano.size - 4 - 5 * k):
            pano[p] = v
            where.setdefault(name, []).append(p)
    return pano.reshape(H, W), where


def check_pano_to_lidar(run, H, W, K, pano, with_inten=True):
    """One call with prefilled outputs.  count exact; column 3 the pixel indices of the non-zero pixels in row-major order, bit
    for bit (+0.0 without intensities); xyz within DIR_K u |range| of the float64 product, NaN / inf where it is; rows at and
    behind count and the guard row behind H W keep the sentinel; the inputs keep their bits.  -> (points, count, largest xyz
    error over the finite rows in units of u |range|)."""
    n = H * W
    assert n < 2 ** 24 and pano.dtype == F32 and pano.shape == (H, W)
    inten = np.arange(n, dtype=F32).reshape(H, W) if with_inten else None
    points, count = np.full((n + 1, 4), SENT, F32), np.array([-7], np.int32)
    got, cnt, pano_after, inten_after = run(pano.copy(), None if inten is None else inten.copy(), H, W, K, points, count)
    assert got.shape == (n + 1, 4) and got.dtype == F32
    idx = np.flatnonzero(pano.reshape(-1) != 0)
    what = f"H={H} W={W} kept={idx.size}"
    assert int(cnt[0]) == idx.size, f"count {int(cnt[0])} != {idx.size} ({what})"
    want3 = idx.astype(F32) if with_inten else np.zeros(idx.size, F32)
    bad = np.flatnonzero(~same_bits(got[:idx.size, 3], want3))
    assert bad.size == 0, f"column 3 ({what}): {bad.size} rows differ, first {bad[:4]}: got {got[bad[:4], 3]}, want {want3[bad[:4]]}"
    assert same_bits(got[idx.size:], np.full((n + 1 - idx.size, 4), SENT, F32)).all(), f"rows behind count were written ({what})"
    assert same_bits(pano_after, pano).all(), "pano was written"
    assert (inten_after is None) == (inten is None) and (inten is None or same_bits(inten_after, inten).all()), "intensities were written"
    if idx.size == 0:
        return got, cnt, 0.0
    r32 = pano.reshape(-1)[idx]
    r64 = r32.astype(F64)
    d64 = pixel_dirs64(H, W, K, idx)
    with np.errstate(all="ignore"):
        want = d64 * r64[:, None]
        xyz = got[:idx.size, :3].astype(F64)
        k = dir_k(K)
        fin = np.isfinite(r64)
        err = np.abs(xyz[fin] - want[fin])
        tol = k * U * np.abs(r64[fin])[:, None] + HALF_SUBNORMAL
        assert (err <= tol).all(), f"xyz ({what}): {(err / np.maximum(np.abs(r64[fin])[:, None], 1e-300)).max() / U:.2f} u |range| > DIR_K = {k:.2f}"
        assert np.isnan(xyz[np.isnan(r64)]).all(), "a NaN range must give NaN coordinates"
        isinf = np.isinf(r64)
        clear = np.abs(d64[isinf]) > k * U
        assert (np.isinf(xyz[isinf]) | ~clear).all() and (xyz[isinf][clear] == want[isinf][clear]).all(), "an inf range: signed inf"
        normal = fin & (np.abs(r64) >= 2.0 ** -100)
        worst = float((np.abs(xyz[normal] - want[normal]) / np.abs(r64[normal])[:, None]).max() / U) if normal.any() else 0.0
    return got, cnt, worst


def check_pano_special(run, H, W, K):
    pano, where = special_image(H, W)
    got, cnt, worst = check_pano_to_lidar(run, H, W, K, pano)
    kept = set(got[:int(cnt[0]), 3].astype(np.int64).tolist())
    for name, ps in where.items():
        for p in ps:
            assert (p in kept) == (name != "neg_zero"), f"{name} at pixel {p}: kept = {p in kept}"
    return worst


# =================================================================================================================================
# 1b. lidar_to_pano
# =================================================================================================================================
LIDAR_FAULTS = (None, "tie_highest", "depth_le")


def lidar_to_pano_f32(points, H, W, K, max_depth, fault=None):
    """l4d_lidar_to_pano restated (lidar_bin_kernel's fp32 steps; the winner = the smallest (range bits, index)).  Without a fault
    this is oracle/convert_ref.py (asserted by the CPU test on every cloud here).  fault 'tie_highest': of equal ranges the highest
    index wins; 'depth_le': dist <= max_depth is kept.  -> pano [H, W], intensities [H, W]."""
    assert fault in LIDAR_FAULTS
    points = np.asarray(points, dtype=F32).reshape(-1, 4)
    fov_up, fov = float(K[0]), float(K[1])
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    with np.errstate(all="ignore"):
        dist = np.sqrt((x * x + y * y) + z * z)
        beta = PI32 - np.arctan2(y, x)
        alpha = np.arctan2(z, np.sqrt(x * x + y * y)) + F32((fov - fov_up) / 180 * np.pi)
        cf = np.rint(beta / F32(2 * np.pi / W))
        rf = np.rint(F32(H) - alpha / F32(fov / 180 * np.pi / H))
        near = dist <= F32(max_depth) if fault == "depth_le" else dist < F32(max_depth)
        ok = near & (rf >= 0) & (rf < H) & (cf >= 0) & (cf < W) & (dist != 0)
    assert dist.dtype == cf.dtype == rf.dtype == F32
    idx = np.flatnonzero(ok)
    pix = rf[idx].astype(np.int64) * W + cf[idx].astype(np.int64)
    order = np.lexsort((-idx if fault == "tie_highest" else idx, dist[idx], pix))
    first = np.ones(order.size, bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win = idx[order][first]
    pano, inten = np.zeros(H * W, F32), np.zeros(H * W, F32)
    pano[pix[order][first]] = dist[win]
    inten[pix[order][first]] = points[win, 3]
    return pano.reshape(H, W), inten.reshape(H, W)


def run_lidar_f32(fault=None):
    def run(points, N, H, W, K, max_depth, pano, inten):
        if H * W:
            p, i = lidar_to_pano_f32(points[:N], H, W, K, max_depth, fault)
            pano[:H * W] = p.reshape(-1)
            if inten is not None:
                inten[:H * W] = i.reshape(-1)
        return pano, inten, points.copy()
    return run


def angles_to_xyz(H, W, K, rf, cf, rng):
    """float64 xyz at fractional pixel (rf, cf) and range rng: the inverse of the projection of utils/convert.py:48-51."""
    fov_up, fov = float(K[0]), float(K[1])
    beta = np.asarray(cf, F64) * (2 * np.pi / W)
    elev = (H - np.asarray(rf, F64)) * (fov / 180 * np.pi / H) - (fov - fov_up) / 180 * np.pi
    phi = np.pi - beta
    rng = np.asarray(rng, F64)
    return np.stack([rng * np.cos(elev) * np.cos(phi), rng * np.cos(elev) * np.sin(phi), rng * np.sin(elev)], -1)


def frac_pixel64(points, H, W, K):
    """float64 fractional pixel (rf, cf) of fp32 points."""
    p = np.asarray(points, F32).astype(F64)
    fov_up, fov = float(K[0]), float(K[1])
    cf = (np.pi - np.arctan2(p[:, 1], p[:, 0])) / (2 * np.pi / W)
    rf = H - (np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1])) + (fov - fov_up) / 180 * np.pi) / (fov / 180 * np.pi / H)
    return rf, cf


CLOUD_SHAPES = [(1, 1, WIDE), (3, 5, WIDE), (8, 16, KITTI), (16, 257, KITTI), (66, 515, MID)]   # run on the device
CLOUD_SHAPES_CPU = CLOUD_SHAPES + [(64, 2048, KITTI), (32, 4096, KITTI)]                          # margin shown here only
MARGIN_MIN = 0.2


def cloud(H, W, K, seed=0, lo=2.0, hi=70.0, shuffle=True):
    """One fp32 point per pixel (module docstring).  -> points [H W, 4] (intensity = 1 + pixel index + seed / 8: distinct and
    exact), pix [H W] the pixel of every point."""
    n = H * W
    r = rng_of(7, H, W, seed)
    pix = np.arange(n)
    row, col = pix // W, pix % W
    dr, dc = r.uniform(-0.25, 0.25, size=n), r.uniform(-0.25, 0.25, size=n)
    dc = np.where(col == 0, np.abs(dc), dc)
    xyz = angles_to_xyz(H, W, K, row + dr, col + dc, r.uniform(lo, hi, size=n))
    pts = np.concatenate([xyz, (1.0 + pix + seed / 8.0)[:, None]], 1).astype(F32)
    if shuffle:
        perm = r.permutation(n)
        pts, pix = pts[perm], pix[perm]
    return np.ascontiguousarray(pts), pix


def cloud_margin(points, pix, H, W, K):
    """Smallest distance (px) of a point's float64 fractional pixel from a bin edge; asserts that it is the intended pixel."""
    rf, cf = frac_pixel64(points, H, W, K)
    assert (np.rint(rf) * W + np.rint(cf) == pix).all()
    return float(min((0.5 - np.abs(rf - np.rint(rf))).min(), (0.5 - np.abs(cf - np.rint(cf))).min()))


def dist_f32(points):
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    with np.errstate(all="ignore"):
        d = np.sqrt((x * x + y * y) + z * z)
    assert d.dtype == F32
    return d


def own_pixel_image(points, pix, H, W):
    """The closed form of an unambiguous cloud: pano[pix] = sqrt_f32((x^2 + y^2) + z^2), intensities[pix] = column 3."""
    pano, inten = np.zeros(H * W, F32), np.zeros(H * W, F32)
    pano[pix], inten[pix] = dist_f32(points), points[:, 3]
    return pano.reshape(H, W), inten.reshape(H, W)


def check_lidar_to_pano(run, points, H, W, K, max_depth, want_pano, want_inten, with_inten=True, what=""):
    """One call with pano and intensities prefilled with NaN and a guard element behind each: EVERY pixel equals the expected
    image bit for bit (empty pixels +0.0), the guards and the points keep their bits; without intensities only pano is written."""
    n, N = H * W, points.shape[0]
    pano = np.full(n + 1, np.nan, F32)
    inten = np.full(n + 1, np.nan, F32)
    pano[n], inten[n] = SENT, SENT
    pts_in = np.ascontiguousarray(points, dtype=F32)
    got_p, got_i, pts_after = run(pts_in.copy(), N, H, W, K, max_depth, pano, inten if with_inten else None)
    for name, got, want in (("pano", got_p, want_pano), ("intensities", got_i, want_inten)):
        if got is None:
            assert name == "intensities" and not with_inten
            continue
        bad = np.flatnonzero(~same_bits(got[:n], np.asarray(want, F32).reshape(-1)))
        assert bad.size == 0, (f"{name} {what} H={H} W={W} N={N}: {bad.size} of {n} pixels differ, first {bad[:4]}: got {got[bad[:4]]}, "
                               f"want {np.asarray(want).reshape(-1)[bad[:4]]}")
        assert same_bits(got[n:], np.array([SENT], F32)).all(), f"{name}: the guard element was written"
    assert same_bits(pts_after, pts_in).all(), "the points were written"
    return got_p[:n].reshape(H, W), None if got_i is None else got_i[:n].reshape(H, W)


def check_unambiguous(run, H, W, K):
    pts, pix = cloud(H, W, K)
    pano, inten = own_pixel_image(pts, pix, H, W)
    assert (pano > 0).all()
    check_lidar_to_pano(run, pts, H, W, K, 80.0, pano, inten, what="unambiguous")
    check_lidar_to_pano(run, pts, H, W, K, 80.0, pano, inten, with_inten=False, what="unambiguous, no intensities")


FILLER = 300          # dropped points (the origin) between contenders: more than one 256-point workgroup apart
CONTEST_SHAPES = [(1, 1, WIDE), (3, 5, WIDE), (8, 16, KITTI)]
CONTEST_K = (2, 3, 5)


def filler(count):
    f = np.zeros((count, 4), F32)
    f[:, 3] = 9000.0 + np.arange(count)
    return f


def contested(H, W, K, k, winner_at):
    """k points in every pixel, in k blocks (one unambiguous cloud each, more than 256 indices apart); block ``winner_at`` has
    the ranges 2 .. 10, the others 20 .. 70.  -> points, expected pano, expected intensities."""
    blocks = []
    for j in range(k):
        pts, pix = cloud(H, W, K, seed=10 + j, lo=2.0 if j == winner_at else 20.0, hi=10.0 if j == winner_at else 70.0)
        pts[:, 3] += F32(1000.0 * j)
        blocks += [pts, filler(FILLER)]
        if j == winner_at:
            want = own_pixel_image(pts, pix, H, W)
    return np.concatenate(blocks[:-1]), want[0], want[1]


def check_contested(run, H, W, K, k):
    """Different ranges: the nearest wins, wherever it stands (first, middle, last block)."""
    for winner_at in sorted({0, k // 2, k - 1}):
        pts, pano, inten = contested(H, W, K, k, winner_at)
        check_lidar_to_pano(run, pts, H, W, K, 80.0, pano, inten, what=f"contested k={k} winner in block {winner_at}")


def check_ties(run, H, W, K, k=2):
    """Equal range bits (identical xyz, other intensities) in k copies: the lowest index wins; the array reversed: the other end."""
    a, pix = cloud(H, W, K, seed=20)
    copies = []
    for j in range(k):
        c = a.copy()
        c[:, 3] += F32(1000.0 * j)
        copies += [c, filler(FILLER)]
    pts = np.concatenate(copies[:-1])
    pano, inten = own_pixel_image(a, pix, H, W)
    check_lidar_to_pano(run, pts, H, W, K, 80.0, pano, inten, what=f"tie of {k}: first copy")
    last = a.copy()
    last[:, 3] += F32(1000.0 * (k - 1))
    check_lidar_to_pano(run, pts[::-1], H, W, K, 80.0, pano, own_pixel_image(last, pix, H, W)[1], what=f"tie of {k}, reversed")


GATE_DEPTHS = (80.0, float(F32(26.9)))
GATE_SHAPE = (8, 16, WIDE)      # +x axis: column W / 2 = 8 and row H fov_up / fov = 2, both pixel centres


def check_range_gate(run, max_depth):
    """Points on the +x axis (dist == |x| exactly): nextafter(max_depth, 0) is kept, max_depth and nextafter(max_depth, inf) are
    dropped -- each alone (N = 1) and the three together."""
    H, W, K = GATE_SHAPE
    md = F32(max_depth)
    assert float(md) == max_depth
    below, above = np.nextafter(md, F32(0)), np.nextafter(md, F32(np.inf))
    mk = lambda xs: np.array([[x, 0.0, 0.0, 5.0 + k] for k, x in enumerate(xs)], F32)
    empty = np.zeros((H, W), F32)
    kept_p, kept_i = empty.copy(), empty.copy()
    kept_p[2, 8], kept_i[2, 8] = below, 5.0
    check_lidar_to_pano(run, mk([below]), H, W, K, max_depth, kept_p, kept_i, what="just inside max_depth")
    check_lidar_to_pano(run, mk([md]), H, W, K, max_depth, empty, empty, what="at max_depth")
    check_lidar_to_pano(run, mk([above]), H, W, K, max_depth, empty, empty, what="just outside max_depth")
    kept_i[2, 8] = 7.0
    check_lidar_to_pano(run, mk([above, md, below]), H, W, K, max_depth, kept_p, kept_i, what="three around max_depth")


def dropped_points(H, W, K):
    """[M, 4] points that must contribute nothing (intensities 7000 + k), with their names."""
    col0 = angles_to_xyz(H, W, K, 1.0, 0.125, 30.0)
    rows = [("origin", (0.0, 0.0, 0.0)), ("up", (0.0, 0.0, 5.0)), ("down", (0.0, 0.0, -5.0)),
            ("above fov_up", angles_to_xyz(H, W, K, -1.0, 3.0, 9.0)), ("below fov_down", angles_to_xyz(H, W, K, float(H), 3.0, 9.0)),
            ("column 0 mirrored", (col0[0], -col0[1], col0[2])), ("column 0, y = -tiny", (-30.0, -1e-30, 0.0))]
    base = angles_to_xyz(H, W, K, 2.0, 5.0, 1.5)   # nearer than every point of the cloud: it would win its pixel
    for axis in range(3):
        for name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("overflow", 1e20), ("-overflow", -1e20)):
            p = list(base)
            p[axis] = v
            rows.append((f"{name} in {'xyz'[axis]}", tuple(p)))
    pts = np.array([list(p) + [7000.0 + k] for k, (_, p) in enumerate(rows)], F32)
    return pts, [n for n, _ in rows]


def check_dropped(run, H, W, K):
    """The unambiguous cloud with every dropped point mixed in: the same image, bit for bit; and each of them alone: empty."""
    pts, pix = cloud(H, W, K, seed=30)
    pano, inten = own_pixel_image(pts, pix, H, W)
    extra, names = dropped_points(H, W, K)
    at = rng_of(8, H, W).randint(0, pts.shape[0] + 1, size=extra.shape[0])
    mixed = np.insert(pts, at, extra, axis=0)
    check_lidar_to_pano(run, mixed, H, W, K, 80.0, pano, inten, what="with dropped points")
    empty = np.zeros((H, W), F32)
    for p, name in zip(extra, names):
        check_lidar_to_pano(run, p[None], H, W, K, 80.0, empty, empty, what=name)


WRITE_SHAPE = (16, 257, KITTI)
WRITE_N = (0, 1, 255, 256, 257)


def check_writes(run):
    """N = 0, 1, 255, 256, 257 points of an unambiguous cloud (every pixel written, empty ones +0.0 in both images), with and
    without intensities; H W = 0 writes nothing."""
    H, W, K = WRITE_SHAPE
    pts, pix = cloud(H, W, K, seed=40)
    for N in WRITE_N:
        pano, inten = own_pixel_image(pts[:N], pix[:N], H, W)
        for with_inten in (True, False):
            check_lidar_to_pano(run, pts[:N], H, W, K, 80.0, pano, inten, with_inten, what=f"N={N}")
    for H0, W0 in ((0, 5), (5, 0), (0, 0)):
        check_lidar_to_pano(run, pts[:7], H0, W0, K, 80.0, np.zeros((H0, W0), F32), np.zeros((H0, W0), F32), what="H W = 0")


EDGE_SHAPE = (8, 16, KITTI)


def check_bin_edges(run):
    """A point at exactly half a pixel in column (then in row), nearer than the cloud's: atan2f and libm may round it to either
    side, so its range (and intensity) must be in exactly one of the two adjacent pixels and the image otherwise unchanged."""
    H, W, K = EDGE_SHAPE
    pts, pix = cloud(H, W, K, seed=50)
    pano, inten = own_pixel_image(pts, pix, H, W)
    for rf, cf in ((2.0, 4.5), (5.1, 11.5), (0.0, 0.5), (2.5, 4.0), (6.5, 9.1), (0.5, 15.0)):
        e = np.concatenate([angles_to_xyz(H, W, K, rf, cf, 1.25), [8000.0]]).astype(F32)
        d = dist_f32(e[None])[0]
        side = lambda v: (int(np.floor(v)), int(np.ceil(v))) if v % 1.0 == 0.5 else (int(np.rint(v)),) * 2
        pair = {r * W + c for r, c in zip(side(rf), side(cf))}
        assert len(pair) == 2
        buf_p, buf_i = np.full(H * W + 1, np.nan, F32), np.full(H * W + 1, np.nan, F32)
        got_p, got_i, _ = run(np.concatenate([pts, e[None]]), pts.shape[0] + 1, H, W, K, 80.0, buf_p, buf_i)
        diff = np.flatnonzero(~same_bits(got_p[:H * W], pano.reshape(-1)) | ~same_bits(got_i[:H * W], inten.reshape(-1)))
        assert diff.size == 1 and int(diff[0]) in pair, f"edge point at ({rf}, {cf}): changed pixels {diff}, allowed one of {sorted(pair)}"
        assert same_bits(got_p[diff], np.array([d])).all() and float(got_i[diff[0]]) == 8000.0
        assert np.isnan(got_p[H * W]) and np.isnan(got_i[H * W])
