"""Edge and exact-lattice tests of the point-cloud preparation kernels on the device (``-m gpu``, MI355X; csrc/pointprep.hip):
ordered compaction at every workgroup edge and beyond 1024 workgroups, the range predicate on each of its boundaries, the
k-nearest mean distance on layouts that make the two-level scan walk, the outlier statistics on a hand-made ``avg``, plane
fitting / counting / masking across hypothesis chunks, and the refusals of the host code.

The cases, the references, the bounds and the check bodies are in tests/pointprep_cases.py; tests/test_pointprep_cases_cpu.py
proves the cases' conditions and runs the same bodies on the restatement of tests/pointprep_ref.py.  Every measured figure is
printed before it is asserted (run with -s)."""
import numpy as np
import pytest
import torch

import pointprep_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)     # (a copy: the cached cases are read-only)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def _api():
    from lidar4d_amd import _prep_lib, ops
    return _prep_lib, ops


def _workspace(n):
    prep, _ = _api()
    return torch.empty(max(4, int(prep.lib().l4dp_compact_workspace(n))), dtype=torch.uint8, device=DEV)


# ---- ``run`` callables of the check bodies: the C ABI with the body's prefilled buffers ------------------------------------------
def run_range(points, n, limits, out, out_index, count):
    prep, ops = _api()
    p = ops._p
    d_pts, d_out, d_index, d_count = dev(points), dev(out), dev(out_index), dev(count)
    ws = _workspace(n)
    prep.call("l4dp_range_filter", p(d_pts), n, float(limits[0]), float(limits[1]), float(limits[2]), float(limits[3]), p(d_out),
              p(d_index), p(d_count), p(ws), ops._stream())
    torch.cuda.synchronize()
    return host(d_out), host(d_index), host(d_count), host(d_pts)


def run_outlier(points, avg, n, std_ratio, out, out_index, count, stats):
    prep, ops = _api()
    p = ops._p
    d_pts, d_avg, d_out, d_index, d_count, d_stats = dev(points), dev(avg), dev(out), dev(out_index), dev(count), dev(stats)
    ws = _workspace(n)
    prep.call("l4dp_outlier_filter", p(d_pts), p(d_avg), n, float(std_ratio), p(d_out), p(d_index), p(d_count), p(d_stats), p(ws),
              ops._stream())
    torch.cuda.synchronize()
    return host(d_out), host(d_index), host(d_count), host(d_stats)


def run_knn(points, k, sort):
    from lidar4d_amd import pointprep
    got = pointprep.knn_mean_distance(dev(points), k, sort=sort)
    assert got.dtype == torch.float32
    return host(got)


def run_score(points, triples, y_gap, threshold):
    from lidar4d_amd import pointprep
    valid, coeffs, counts = pointprep.plane_score(dev(points), triples, threshold, y_gap=y_gap)
    return host(valid), host(coeffs), host(counts)


def run_mask(points, coeffs, threshold, mask):
    from lidar4d_amd import pointprep
    return host(pointprep.plane_mask(dev(points), coeffs, threshold, mask=dev(mask)))


# =================================================================================================================================
# 1. ordered compaction: compact_count_kernel, compact_emit_kernel
# =================================================================================================================================
@pytest.mark.parametrize("n", pc.COMPACT_N)
def test_compaction_patterns_order_count_index_and_untouched_rows(n):
    """keep-all, keep-none, first only, last only, the last lane of every workgroup, lane 0 of every wavefront, alternating and a
    random half: out == pts[mask] bit for bit, count, out_index, nothing written behind count -- with and without out_index."""
    from lidar4d_amd import pointprep
    for pattern in pc.COMPACT_PATTERNS:
        kept = pc.check_compaction(run_range, n, pattern)
        keep = pc.keep_pattern(n, pattern)
        pts = pc.compact_points(keep)
        assert pc.same_bits(host(pointprep.range_filter(dev(pts))), pts[keep]).all()      # the public wrapper
        print(f"compaction n={n} {pattern}: kept {kept}")


def test_compaction_second_trip_of_the_prefix_loop():
    """1025 * 1024 + 1 points, a random half kept: 1026 workgroups, the last of which sums the 1025 counts in front of it in two
    trips of its strided loop."""
    kept = pc.check_compaction(run_range, pc.COMPACT_BIG, "random_half", seed=1)
    print(f"compaction n={pc.COMPACT_BIG} random half: kept {kept}")


def test_compaction_twice_gives_the_same_bits():
    keep = pc.keep_pattern(3073, "random_half")
    pts = pc.compact_points(keep)
    a = pc.check_range_filter(run_range, pts, keep)
    b = pc.check_range_filter(run_range, pts, keep)
    assert pc.same_bits(a, b).all()


# =================================================================================================================================
# 2. the range predicate on its boundaries
# =================================================================================================================================
def test_range_predicate_on_every_boundary():
    """A point on each boundary of the nine inequalities and its neighbour to either side, NaN and infinite coordinates, the
    interior of the ego box: the float32 evaluation of pointprep_ref.range_filter_mask (== its float64 evaluation: CPU test) --
    every point alone, and the table in one call in both orders."""
    from lidar4d_amd import pointprep
    kept = pc.check_boundaries(run_range)
    for limits, names, pts, mask in pc.boundary_clouds():
        got = host(pointprep.range_filter(dev(pts), dist_min=limits[0], dist_max=limits[1], z_limit=(limits[2], limits[3])))
        assert pc.same_bits(got, pts[mask]).all()
        print(f"range predicate, limits {limits}: {len(names)} boundary points, {int(mask.sum())} kept")
    assert kept > 0


# =================================================================================================================================
# 3. k-nearest mean distance: knn_soa_kernel, knn_mean_dist_kernel
# =================================================================================================================================
@pytest.mark.parametrize("name", pc.KNN_CASES)
def test_knn_mean_distance_layouts(name):
    """Integer lattice (exact ties at every k), interleaved halves (queries of the first group walk up, those of the last walk
    down), padding edges, a far point that collapses the Morton keys, zero extent, identical points: sort=True and sort=False,
    k in {1, 2, 7, 63, 64}, against the float64 brute reference within KNN_RTOL; exactly 0 where the reference is 0."""
    worst = pc.check_knn(run_knn, name)
    print(f"knn {name}: every k, both orders: largest relative error {worst:.3e}")


def test_knn_mean_distance_interleaved_is_bit_reproducible():
    pts = pc.knn_case("interleaved")[0]
    for sort in (True, False):
        a, b = run_knn(pts, 64, sort), run_knn(pts, 64, sort)
        assert pc.same_bits(a, b).all()


# =================================================================================================================================
# 4. outlier statistics and the threshold compaction, without the k-nearest kernel
# =================================================================================================================================
@pytest.mark.parametrize("n", pc.OUTLIER_N)
def test_outlier_statistics_on_a_synthetic_avg(n):
    """(mu, sd, threshold) against numpy float64 on the same float32 values within 1e-10; the kept rows are flatnonzero(avg < thr)
    exactly (no value within 1e-6 thr of it: CPU test).  All values equal: (a, 0, a) exactly, nothing kept."""
    pc.check_outlier_mixed(run_outlier, n)
    pc.check_outlier_equal(run_outlier, n)


def test_outlier_statistics_single_value():
    pc.check_outlier_single(run_outlier)


def test_remove_statistical_outlier_degenerate_clouds():
    """200 identical points (every mean distance 0, threshold 0, strict <) and one point (sd = NaN): nothing is kept."""
    from lidar4d_amd import pointprep
    for pts in (np.tile(np.array([[1.25, -3.5, 0.75]], F32), (200, 1)), np.array([[1.25, -3.5, 0.75]], F32)):
        kept, ind, avg, stats = pointprep.remove_statistical_outlier(dev(pts), 64, 3.0, return_stats=True)
        print(f"remove_statistical_outlier on {len(pts)} identical points: stats {host(stats).tolist()}, kept {kept.shape[0]}")
        assert kept.shape == (0, 3) and kept.dtype == torch.float32 and ind.shape == (0,) and ind.dtype == torch.int64
        assert not host(avg).any()


# =================================================================================================================================
# 5. planes: plane_fit_kernel, plane_count_kernel, plane_mask_kernel
# =================================================================================================================================
@pytest.mark.parametrize("n_points,n_triples", [(1000, 513), (1000, 300), (1000, 257), (257, 513), (63, 513), (1, 513)])
def test_plane_scoring_across_hypothesis_chunks(n_points, n_triples):
    """513 hypotheses = chunks of 256, 256 and 1 over the LDS counters (300: a short second chunk; 257: a chunk of one after a
    full one).  valid and coeffs bit-equal to pointprep_ref.score_batch, counts within the band of the float64 counts, rejected
    hypotheses 0 wherever they sit in a chunk, a second launch the same counts."""
    pc.check_plane_score(run_score, n_points, n_triples)


def test_plane_rejection_rules_at_their_edges():
    """A y gap of exactly 3 is accepted and 2.5 is not; a repeated row, a zero component of p1 - p0 and a collinear triple are
    rejected; a duplicate point under another index gives the same plane."""
    pc.check_plane_rejection(run_score)


@pytest.mark.parametrize("n", pc.MASK_N)
def test_plane_mask_is_the_or_of_the_single_plane_masks(n):
    """n_planes in {0, 1, 6, 7}: mask == prefill | OR of the single-plane masks, whose sums are the scoring kernel's counts."""
    pc.check_plane_mask(run_mask, run_score, n)


# =================================================================================================================================
# 6. refusals: arguments the host code rejects before any launch
# =================================================================================================================================
def test_refusals_leave_every_buffer_alone():
    prep, ops = _api()
    p, lib = ops._p, prep.lib()
    n = 100
    pts = pc.compact_points(np.ones(n, bool))
    d_pts = dev(pts)
    out, index, count = dev(np.full((n, 3), pc.SENT, F32)), dev(np.full(n, pc.ISENT, np.int32)), dev(np.array([pc.ISENT], np.int32))
    avg, stats = dev(np.full(n, pc.SENT, F32)), dev(np.full(3, -1.0, F64))
    tri = dev(np.array([[0, 50, 99]], np.int32))
    valid, coeffs, counts = dev(np.array([pc.ISENT], np.int32)), dev(np.full((1, 4), pc.SENT, F32)), dev(np.array([pc.ISENT], np.int32))
    mask = dev(np.full(n, 0x55, np.uint8))
    knn_ws = torch.zeros(int(lib.l4dp_knn_workspace(n)), dtype=torch.uint8, device=DEV)
    ws = _workspace(n)
    before = [t.clone() for t in (d_pts, out, index, count, avg, stats, valid, coeffs, counts, mask, knn_ws)]
    s = ops._stream()
    calls = {
        "knn k=0": ("l4dp_knn_mean_dist", (p(d_pts), n, 0, None, p(avg), p(knn_ws), s)),
        "knn k=65": ("l4dp_knn_mean_dist", (p(d_pts), n, 65, None, p(avg), p(knn_ws), s)),
        "knn n<0": ("l4dp_knn_mean_dist", (p(d_pts), -1, 64, None, p(avg), p(knn_ws), s)),
        "range n<0": ("l4dp_range_filter", (p(d_pts), -1, 1.0, 50.0, -2.5, 4.0, p(out), p(index), p(count), p(ws), s)),
        "range null count": ("l4dp_range_filter", (p(d_pts), n, 1.0, 50.0, -2.5, 4.0, p(out), p(index), None, p(ws), s)),
        "outlier n<0": ("l4dp_outlier_filter", (p(d_pts), p(avg), -1, 3.0, p(out), p(index), p(count), p(stats), p(ws), s)),
        "outlier null count": ("l4dp_outlier_filter", (p(d_pts), p(avg), n, 3.0, p(out), p(index), None, p(stats), p(ws), s)),
        "score n<0": ("l4dp_plane_score", (p(d_pts), -1, p(tri), 1, 3.0, 0.15, p(valid), p(coeffs), p(counts), s)),
        "score n_hyp<0": ("l4dp_plane_score", (p(d_pts), n, p(tri), -1, 3.0, 0.15, p(valid), p(coeffs), p(counts), s)),
        "mask n<0": ("l4dp_plane_mask", (p(d_pts), -1, p(coeffs), 1, 0.15, p(mask), s)),
        "mask n_planes<0": ("l4dp_plane_mask", (p(d_pts), n, p(coeffs), -1, 0.15, p(mask), s)),
    }
    for what, (name, args) in calls.items():
        status = getattr(lib, name)(*args)
        text = lib.l4dp_last_error().decode()
        print(f"{what}: status {status}, '{text}'")
        assert status != 0, what
        assert text.startswith(name + ":"), (what, text)
        with pytest.raises(prep.HipExtensionError, match=name):
            prep.call(name, *args)
    torch.cuda.synchronize()
    for t, b in zip((d_pts, out, index, count, avg, stats, valid, coeffs, counts, mask, knn_ws), before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
