"""CPU tests of tests/pointprep_cases.py: every case is what it claims to be, and every check body that
tests/test_gpu_pointprep_edges.py applies to a kernel passes on the restatement of tests/pointprep_ref.py.  The reference alone:
nothing here runs HIP code.  The figures the conditions rest on are printed before they are asserted (run with -s)."""
import numpy as np
import pytest
import torch

import pointprep_cases as pc
import pointprep_ref as ref

F32, F64 = np.float32, np.float64


# ---- 1. compaction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.COMPACT_N)
def test_compaction_cases_are_exact_distinct_and_far_from_every_limit(n):
    for pattern in pc.COMPACT_PATTERNS:
        keep = pc.keep_pattern(n, pattern)
        pts = pc.compact_points(keep)
        assert np.array_equal(ref.range_filter_mask(pts), keep)
        assert np.array_equal(pc.range_mask64(pts, pc.DEFAULT_LIMITS), keep)
        assert len({r.tobytes() for r in pts[keep]}) == keep.sum()
        assert pc.check_compaction(pc.run_range_ref, n, pattern) == keep.sum()
    assert pc.keep_pattern(n, "none").sum() == 0 and pc.keep_pattern(n, "all").sum() == n
    assert pc.keep_pattern(n, "first").sum() == 1 and pc.keep_pattern(n, "last")[n - 1]
    assert pc.keep_pattern(n, "lane_1023").sum() == n // 1024


def test_large_compaction_case_reaches_the_second_trip_of_the_prefix_loop():
    n = pc.COMPACT_BIG
    assert -(-n // pc.PC_THREADS) - 1 > pc.PC_THREADS          # the last workgroup has more than 1024 in front of it
    keep = pc.keep_pattern(n, "random_half", seed=1)
    pts = pc.compact_points(keep)
    d = np.sqrt((pts[keep].astype(F64) ** 2).sum(1))
    print(f"large compaction case: n={n}, kept {keep.sum()}, kept distances {d.min():.3f} .. {d.max():.3f}, y up to {pts[:, 1].max()}")
    assert 10.0 <= d.min() and d.max() < 43.0
    assert np.array_equal(ref.range_filter_mask(pts), keep)
    bits = np.ascontiguousarray(pts[keep]).view(np.uint32).astype(np.uint64)
    assert not bits[:, 2].any() and len(np.unique((bits[:, 0] << np.uint64(32)) | bits[:, 1])) == keep.sum()    # distinct rows
    # the counts of the second trip matter: workgroups 1024.. keep something
    assert keep[1024 * pc.PC_THREADS:].sum() > 0 and 0 < keep[:pc.PC_THREADS].sum() < pc.PC_THREADS
    pc.check_compaction(pc.run_range_ref, n, "random_half", seed=1)


# ---- 2. range predicate ----------------------------------------------------------------------------------------------------------
def test_boundary_table_is_unambiguous_and_covers_every_inequality():
    table = pc.boundary_table()
    names = [n for n, _, _ in table]
    for limits, cloud_names, pts, mask in pc.boundary_clouds():
        m64 = pc.range_mask64(pts, limits)
        for n, p, a, b in zip(cloud_names, pts, mask, m64):
            print(f"{limits[0]:g}..{limits[1]:g}  {n:34s} {p!s:42s} kept {bool(a)}")
        assert np.array_equal(mask, m64), [n for n, a, b in zip(cloud_names, mask, m64) if a != b]
        by = dict(zip(cloud_names, mask))
        # each boundary: the point on it and its two neighbours get the verdicts of >=, <=, >, <
        for stem, on, below, above in (("dist_min (3,4,0)", 1, 0, 1), ("dist_min (3,4,0) y", 1, 0, 1), ("dist_min (-3,-4,0)", 1, 0, 1),
                                       ("dist_min (5,0,0)", 1, 0, 1), ("dist_min (0,-5,0)", 1, 0, 1), ("dist_max (30,40,0)", 1, 1, 0),
                                       ("dist_max (30,40,0) y", 1, 1, 0), ("dist_max (50,0,0)", 1, 1, 0), ("dist_max (0,50,0)", 1, 1, 0),
                                       ("dist_max (-50,0,0)", 1, 1, 0), ("dist_min=1 (0,1,0)", 1, 0, 1), ("dist_min=1 (0,-1,0)", 1, 0, 1),
                                       ("dist_min=1 (1,0,0) in ego", 0, 0, 0), ("z_min", 0, 0, 1), ("z_max", 0, 1, 0),
                                       ("ego x=2", 1, 0, 1), ("ego x=-2", 1, 1, 0), ("ego y=1", 1, 0, 1), ("ego y=-1", 1, 1, 0),
                                       ("ego z=2", 1, 0, 1), ("ego z=-2", 1, 1, 0)):
            if stem + " =" in by:
                assert (by[stem + " ="], by[stem + " -"], by[stem + " +"]) == (on, below, above), stem
        for n in cloud_names:
            if "nan" in n or "inf" in n or n.startswith("ego interior"):
                assert not by[n], n
    for stem in ("dist_min (3,4,0)", "dist_max (30,40,0)", "z_min", "z_max", "ego x=2", "ego x=-2", "ego y=1", "ego y=-1", "ego z=2",
                 "ego z=-2"):
        assert {stem + " =", stem + " -", stem + " +"} <= set(names), stem
    # one ulp where the module says so: the faces, the z limits and the axis points
    for n, _, p in table:
        for stem, axis, v in (("ego x=2", 0, 2), ("ego y=-1", 1, -1), ("ego z=2", 2, 2), ("z_min", 2, -2.5), ("z_max", 2, 4),
                              ("dist_min (5,0,0)", 0, 5), ("dist_max (0,50,0)", 1, 50)):
            if n in (stem + " -", stem + " +"):
                assert p[axis] in (np.nextafter(F32(v), F32(-np.inf)), np.nextafter(F32(v), F32(np.inf))), n
    assert pc.check_boundaries(pc.run_range_ref) > 0


# ---- 3. k-nearest mean distance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.KNN_CASES)
def test_knn_reference_is_the_brute_restatement_and_equals_the_kdtree(name):
    pts, d2 = pc.knn_case(name)
    n = len(pts)
    assert pts.dtype == F32 and d2.shape == (n, min(pc.KNN_REF_COLS, n)) and (d2[:, 0] == 0).all()
    for k in (7, 64) if len(pc.knn_ks(name)) > 1 and n <= 5000 else (64,):     # (3 s per k on the 9000 points)
        assert np.array_equal(pc.knn_want(d2, k), ref.knn_mean_distance(pts, k, method="brute")), k     # bit for bit
    worst = pc.check_knn(pc.run_knn_kdtree, name, rtol=1e-9, sorts=(True,))     # (the kd-tree has no visiting order)
    print(f"knn case {name}: n={n}, brute against kd-tree: largest relative difference {worst:.3e}")


def test_knn_cases_have_the_layouts_they_claim():
    from scipy.spatial import cKDTree
    # lattice: every squared distance an exact integer, two groups of 64 batches, n no multiple of 64
    pts, d2 = pc.knn_case("lattice")
    assert len(pts) == 4913 and len(pts) % 64 and -(-len(pts) // 64) == 77 and np.array_equal(d2, np.rint(d2))
    a, b = pc.knn_case("lattice_shuffled")
    assert sorted(map(bytes, a)) == sorted(map(bytes, pts)) and not np.array_equal(a, pts)
    # interleaved halves: the nearest other point is 4500 rows away; 141 batches in three groups
    pts, d2 = pc.knn_case("interleaved")
    h = pc.INTERLEAVED_HALF
    _, nn = cKDTree(pts.astype(F64)).query(pts.astype(F64), k=2)
    assert len(pts) == 2 * h and -(-len(pts) // 64) == 141 and np.array_equal(np.abs(nn[:, 1] - np.arange(2 * h)), np.full(2 * h, h))
    assert len({r.tobytes() for r in pts}) == 2 * h and d2[:, 1].max() < 0.0011 ** 2
    # far point: one key for everything but the far point, which sorts last -- the Morton order is the input order
    pts, _ = pc.knn_case("far_point")
    from lidar4d_amd import pointprep
    order = pointprep._morton_order(torch.from_numpy(pts.copy())).numpy()
    assert np.array_equal(order, np.concatenate([np.delete(np.arange(len(pts)), pc.FAR_ROW), [pc.FAR_ROW]]))
    # zero extent
    assert not pc.knn_case("flat")[0][:, 2].any() and not pc.knn_case("line_x")[0][:, 1:].any()
    p = pc.knn_case("line_diagonal")[0].astype(F64)
    assert np.linalg.matrix_rank(p - p[0], tol=1e-4) == 1
    # identical points: reference exactly 0
    assert not pc.knn_case("identical_200")[1].any()
    pts, d2 = pc.knn_case("copies_70x64")
    assert len(pts) == 4480 and not d2[:, :64].any() and (d2[:, 64] > 0).all()
    # exact ties AT the k-th distance (the k-th and the (k+1)-th smallest are equal) for every k, in an exact-integer case or in a
    # cloud of copies
    for k in pc.KNN_KS:
        tied = sum(int(np.count_nonzero(pc.knn_case(c)[1][:, k - 1] == pc.knn_case(c)[1][:, k])) for c in ("lattice", "copies_70x64"))
        print(f"k={k}: {tied} rows with a tie at the k-th distance")
        assert tied > 0
    # padding edges: the last group of 4097 and 8193 points is one real batch and 63 empty boxes
    for n in (4097, 8193):
        assert -(-n // 64) % 64 == 1
    assert [len(pc.knn_case(f"pad_{n}")[0]) for n in pc.KNN_PAD_N] == list(pc.KNN_PAD_N)


# ---- 4. outlier statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.OUTLIER_N)
def test_outlier_values_keep_clear_of_the_threshold(n):
    avg = pc.outlier_avg(n)
    mu, sd, thr = pc.stats64(avg)
    gap = np.abs(avg.astype(F64) - thr).min() / thr
    removed = np.count_nonzero(~(avg.astype(F64) < thr))
    print(f"outlier case n={n}: mu {mu:.6f} sd {sd:.6f} thr {thr:.6f}, nearest value {gap:.3e} thr away, removed {removed}")
    assert gap > 1e-6
    assert np.isclose(thr, ref.outlier_threshold(avg), rtol=1e-14)
    assert (removed > 0) == (n >= 100) and removed < n
    err = pc.check_outlier_mixed(pc.run_outlier_ref, n)
    assert (err <= 1e-14).all()
    pc.check_outlier_equal(pc.run_outlier_ref, n)


def test_outlier_single_value_follows_the_restatement():
    pc.check_outlier_single(pc.run_outlier_ref)
    keep, avg, thr = ref.statistical_outlier(np.zeros((1, 3), F32), method="brute")
    assert not keep.any() and np.isnan(thr)
    keep, avg, thr = ref.statistical_outlier(np.tile(np.array([[1.0, 2.0, 3.0]], F32), (200, 1)), method="brute")
    assert not keep.any() and thr == 0.0


# ---- 5. planes -------------------------------------------------------------------------------------------------------------------
def test_plane_hypotheses_band_is_small_and_every_chunk_position_is_covered():
    data, tri = pc.plane_cloud(), pc.plane_triples()
    assert tri.shape == (513, 3) and all((len(set(t)) == 3) != (h in pc.FORCED_INVALID) for h, t in enumerate(tri.tolist()))
    for n_points in pc.PLANE_POINT_COUNTS:
        valid, coeffs, counts = pc.score_ref(data[:n_points], tri)
        c64, band = pc.counts64(data[:n_points], coeffs, valid)
        diff = np.abs(counts - c64)
        print(f"plane case, {n_points} points: {valid.sum()} of {len(tri)} hypotheses valid, largest band {band.max()}, fp32 restatement "
              f"against float64 counts: largest difference {diff.max()}, largest count {counts.max()}")
        assert band.max() <= 0.01 * n_points                      # the condition of the count comparison (63 points: empty)
        assert (diff <= band).all()
        assert not valid[list(pc.FORCED_INVALID)].any()
        if n_points == 1000:
            assert valid[256] and counts[256] > 0 and valid[512] and counts[512] > 0
            assert valid[:256].sum() > 100 and counts[:256].max() > 100       # chunk one leaves counters worth resetting
            full = (valid, coeffs)
        elif n_points > 1:
            same = np.flatnonzero(valid)
            assert same.size > 20 and np.array_equal(coeffs[same], full[1][same])   # the same planes on fewer points
            assert not valid[(tri >= n_points).any(axis=1)].any()
        else:
            assert not valid.any()
    for n_triples in pc.TRIPLE_COUNTS:
        assert pc.check_plane_score(pc.run_score_ref, 1000, n_triples)[0] > 0
    pc.check_plane_score(pc.run_score_ref, 63, 513)


def test_plane_rejection_cloud_is_exact():
    pc.check_plane_rejection(pc.run_score_ref)
    # exact: the float64 fit of the fp32 cloud has the same coefficients
    for t, ok in zip(pc.REJECT_TRIPLES, pc.REJECT_VALID):
        co64 = ref.sample_model(pc.REJECT_CLOUD.astype(F64), list(t))
        co32 = ref.sample_model(pc.REJECT_CLOUD, list(t))
        assert (co64 is not None) == (co32 is not None) == bool(ok)
        if ok:
            assert np.array_equal(co64, co32.astype(F64))


@pytest.mark.parametrize("n", pc.MASK_N)
def test_plane_mask_body_passes_on_the_restatement(n):
    coeffs, counts, hyp = pc.mask_planes()
    assert coeffs.shape == (7, 4) and (counts > 0).all()
    pc.check_plane_mask(pc.run_mask_ref, pc.run_score_ref, n)
