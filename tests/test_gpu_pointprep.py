"""GPU tests of lidar4d_amd.pointprep (csrc/pointprep.hip) against the float64 restatement of tests/pointprep_ref.py and the
reference-written fixture tests/golden/point_removal.npz.  Every figure is printed before it is asserted (run with -s)."""
import os
import random

import numpy as np
import pytest
import torch

import pointprep_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.15           # the reference's RANSAC distance threshold in point_removal
PLANE_BAND = 1e-4    # metres: ten times the fp32 error of a plane distance at 50 m range (about 1e-5 m)
OUTLIER_BAND = 1e-4  # relative to the outlier threshold
KNN_RTOL = 1e-5      # fp32 inputs on both sides; the device adds at most about 70 roundings of 2^-24 per value (4e-6)


@pytest.fixture(scope="module")
def fx():
    f = dict(np.load(os.path.join(ROOT, "tests", "golden", "point_removal.npz"), allow_pickle=False))
    f["filtered"] = f["cloud"][f["rf_index"]]
    n = int(f["n_filtered"])
    f["inliers"] = np.unpackbits(f["inliers"], axis=-1)[..., :n].astype(bool)
    return f


@pytest.fixture(scope="module")
def big_cloud():
    return ref.range_filter(ref.make_cloud(64, 1024, seed=1))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(sub, full):
    """Boolean mask over the rows of ``full`` [N,3] that appear in ``sub`` (rows compared bit for bit; ``full`` has no duplicates)."""
    index = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(full))}
    assert len(index) == len(full), "duplicate rows"
    mask = np.zeros(len(full), bool)
    for r in np.ascontiguousarray(sub):
        mask[index[r.tobytes()]] = True
    assert mask.sum() == len(sub)
    return mask


def _knn_check(pts, k=64, label=""):
    from lidar4d_amd import pointprep
    got = pointprep.knn_mean_distance(_dev(pts), k).cpu().numpy()
    want = ref.knn_mean_distance(pts, k)
    err = np.abs(got - want) / np.maximum(want, 1e-300)
    err[want == 0] = np.abs(got[want == 0])
    print(f"knn {label}: n={len(pts)} k={k} max rel err {err.max():.3e}")
    assert got.dtype == np.float32 and np.all(np.abs(got - want) <= KNN_RTOL * want)
    return got


def test_range_filter_equals_reference_fixture(fx):
    from lidar4d_amd import pointprep
    got = pointprep.range_filter(_dev(fx["cloud"])).cpu().numpy()
    assert np.array_equal(got, fx["filtered"])  # same rows, same order
    assert pointprep.range_filter(torch.zeros(0, 3, device=DEV)).shape == (0, 3)


def test_knn_mean_distance_fixture_cloud(fx):
    _knn_check(fx["filtered"], label="fixture 32x512")


def test_knn_mean_distance_64x1024_frame(big_cloud):
    _knn_check(big_cloud, label="64x1024")


def test_knn_mean_distance_edge_cases(fx):
    from lidar4d_amd import pointprep
    data = fx["filtered"]
    _knn_check(data[:40], label="n < 64")                     # all of them
    _knn_check(data[:64], label="n = 64")
    _knn_check(data[:1], label="n = 1")
    _knn_check(data[:1001], label="n not a multiple of 64")
    _knn_check(data[:1001], k=16, label="k = 16")
    _knn_check(data[:130], k=1, label="k = 1")                # the point itself: 0
    dup = np.concatenate([data[:300]] * 3 + [data[:70]] * 70)  # ties at the k-th distance, and points with 64 copies (mean 0)
    _knn_check(dup, label="duplicates")
    # input order or Morton order: the same neighbours
    a = pointprep.knn_mean_distance(_dev(data[:5000]), 64, sort=False).cpu().numpy()
    b = pointprep.knn_mean_distance(_dev(data[:5000]), 64, sort=True).cpu().numpy()
    assert np.allclose(a, b, rtol=2 * KNN_RTOL, atol=0)
    with pytest.raises(ValueError):
        pointprep.knn_mean_distance(_dev(data[:100]), 65)


def test_knn_mean_distance_is_bit_reproducible(big_cloud):
    from lidar4d_amd import pointprep
    pts = _dev(big_cloud)
    a = pointprep.knn_mean_distance(pts, 64)
    b = pointprep.knn_mean_distance(pts, 64)
    assert torch.equal(a, b)


def _outlier_check(pts, label):
    from lidar4d_amd import pointprep
    kept, ind, avg, stats = pointprep.remove_statistical_outlier(_dev(pts), 64, 3.0, return_stats=True)
    keep_ref, avg_ref, thr_ref = ref.statistical_outlier(pts, 64, 3.0)
    got = np.zeros(len(pts), bool)
    got[ind.cpu().numpy()] = True
    band = np.abs(avg_ref - thr_ref) <= OUTLIER_BAND * thr_ref
    mu, sd, thr = stats.cpu().numpy()
    print(f"outlier {label}: n={len(pts)} removed gpu {np.count_nonzero(~got)} ref {np.count_nonzero(~keep_ref)}, in band "
          f"{band.sum()}, differing {np.count_nonzero(got != keep_ref)}, thr gpu {thr:.9g} ref {thr_ref:.9g}")
    assert torch.equal(kept, _dev(pts)[ind])                         # order preserved, rows intact
    assert bool((ind[1:] > ind[:-1]).all())
    assert band.sum() <= 1e-3 * len(pts)
    assert np.array_equal(got[~band], keep_ref[~band])
    assert abs(thr - thr_ref) <= 1e-5 * thr_ref and abs(mu - avg_ref.mean()) <= 1e-5 * mu
    return got


def test_outlier_keep_mask_fixture_cloud(fx):
    _outlier_check(fx["filtered"], "fixture 32x512")


def test_outlier_keep_mask_64x1024_frame(big_cloud):
    _outlier_check(big_cloud, "64x1024")


def test_outlier_filter_small_clouds(fx):
    from lidar4d_amd import pointprep
    kept, ind = pointprep.remove_statistical_outlier(_dev(fx["filtered"][:40]))
    keep_ref, _, _ = ref.statistical_outlier(fx["filtered"][:40])
    assert np.array_equal(ind.cpu().numpy(), np.flatnonzero(keep_ref))
    kept, ind = pointprep.remove_statistical_outlier(torch.zeros(0, 3, device=DEV))
    assert kept.shape == (0, 3) and ind.numel() == 0


def test_plane_scoring_on_every_fixture_sample(fx):
    from lidar4d_amd import pointprep
    data, samples = fx["filtered"], fx["samples"]
    pts = _dev(data)
    valid, coeffs, counts = pointprep.plane_score(pts, samples, THR)
    valid, coeffs, counts = valid.cpu().numpy(), coeffs.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(valid.astype(bool), fx["sample_valid"])
    assert coeffs.tobytes() == fx["sample_model"].tobytes()          # bit-equal, zeros where rejected
    assert np.all(counts[~fx["sample_valid"]] == 0)
    data64 = data.astype(np.float64)
    worst = 0
    for h in np.flatnonzero(fx["sample_valid"]):
        d = ref.plane_distance(data64, fx["sample_model"][h].astype(np.float64))
        band = np.abs(d - THR) < PLANE_BAND
        want = d < THR
        worst = max(worst, abs(int(counts[h]) - int(want.sum())))
        assert abs(int(counts[h]) - int(want.sum())) <= band.sum(), (h, counts[h], want.sum(), band.sum())
        mask = pointprep.plane_mask(pts, coeffs[h], THR).cpu().numpy().astype(bool)
        assert np.array_equal(mask[~band], want[~band]), h
        assert abs(int(mask.sum()) - int(counts[h])) == 0            # the two kernels agree with each other
    print(f"plane scoring: {len(samples)} samples, largest |count_gpu - count_f64| = {worst}, "
          f"largest |count_gpu - count_reference_fp32| = {np.abs(counts - fx['sample_count']).max()}")
    # out-of-range rows are rejected, not read
    v, c, n = pointprep.plane_score(pts, [[0, 1, len(data)], [-1, 2, 3]], THR)
    assert v.tolist() == [0, 0] and n.tolist() == [0, 0]


def test_estimate_plane_follows_the_reference(fx):
    from lidar4d_amd import pointprep
    data = fx["filtered"]
    h = int(np.flatnonzero(fx["sample_valid"])[0])
    tri = data[fx["samples"][h]]
    co = pointprep.estimate_plane(_dev(tri), normalize=False)
    assert co.cpu().numpy().tobytes() == fx["sample_model"][h].tobytes()
    con = pointprep.estimate_plane(_dev(tri)).cpu().numpy()                # normalize=True: unit normal of the same plane
    n64 = fx["sample_model"][h][:3].astype(np.float64)
    n64 /= np.linalg.norm(n64)
    assert np.allclose(con, np.append(n64, -(n64 @ tri[0].astype(np.float64))), rtol=1e-4, atol=1e-5)
    flat = tri.copy()
    flat[1, 2] = flat[0, 2]                                           # a zero component of p1 - p0
    assert pointprep.estimate_plane(_dev(flat)) is None


def _ground_of_runs(fx, si):
    return fx["inliers"][si].any(0) & (fx["filtered"][:, 2] < -1)


def _reference_spread(fx):
    g = [_ground_of_runs(fx, s) for s in range(3)]
    return max(ref.jaccard_distance(g[a], g[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def test_six_ransac_runs_on_the_fixture_cloud_follow_the_reference(fx):
    """my_ransac on the cloud the reference's runs worked on, random.seed(0): the generator is consumed as the reference consumes it
    (same state after six runs unless a count inside the band changed a decision), and the ground set lies within twice the
    reference's own seed-to-seed spread of its seed-0 ground set."""
    from lidar4d_amd import pointprep
    data = fx["filtered"]
    pts = _dev(data)
    random.seed(0)
    union = np.zeros(len(data), bool)
    same_models = 0
    for run in range(6):
        idx, model = pointprep.my_ransac(pts, distance_threshold=THR)
        assert idx.dtype == torch.int64 and model.shape == (4,)
        union[idx.cpu().numpy()] = True
        same_models += model.cpu().numpy().tobytes() == fx["models"][0, run].tobytes()
    after = random.random()
    ground = union & (data[:, 2] < -1)
    dist, spread = ref.jaccard_distance(ground, _ground_of_runs(fx, 0)), _reference_spread(fx)
    print(f"six runs, seed 0: {same_models}/6 models bit-equal to the reference's, generator in step: {after == fx['rand_after'][0]}, "
          f"Jaccard distance to the reference's ground {dist:.3e}, reference spread {spread:.3e}")
    assert dist <= 2 * spread
    # an explicit generator: the module-level one is left alone
    random.seed(5)
    pointprep.my_ransac(pts, distance_threshold=THR, rng=random.Random(0))
    random_after = random.random()
    random.seed(5)
    assert random_after == random.random()


@pytest.fixture(scope="module")
def removal_run(fx):
    from lidar4d_amd import pointprep
    random.seed(0)
    points, ground, models = pointprep.point_removal(_dev(fx["cloud"]), return_models=True)
    return points.cpu().numpy(), ground.cpu().numpy(), models.cpu().numpy(), random.random()


def test_point_removal_equals_restatement_from_its_own_planes(fx, removal_run):
    """A count that differs by one inside the band can legitimately select another, equally good plane, so the expected output
    is re-derived from the planes the run itself chose: union of their inlier masks, z < -1, outlier removal."""
    from lidar4d_amd import pointprep
    points, ground, models, _ = removal_run
    rf = fx["filtered"]
    assert models.shape == (6, 4) and points.dtype == np.float32 and ground.dtype == np.float32
    # stage 1 (deterministic, so this is the cloud the run's RANSAC saw)
    pc1_t, ind1 = pointprep.remove_statistical_outlier(pointprep.range_filter(_dev(fx["cloud"])), 64, 3.0)
    pc1 = pc1_t.cpu().numpy()
    keep1, avg1, thr1 = ref.statistical_outlier(rf)
    band1 = np.abs(avg1 - thr1) <= OUTLIER_BAND * thr1
    got1 = np.zeros(len(rf), bool)
    got1[ind1.cpu().numpy()] = True
    assert band1.sum() <= 1e-3 * len(rf) and np.array_equal(got1[~band1], keep1[~band1])
    # planes -> ground
    d = np.stack([ref.plane_distance(pc1.astype(np.float64), m.astype(np.float64)) for m in models])
    want_ground = (d < THR).any(0) & (pc1[:, 2] < -1)
    band_p = (np.abs(d - THR) < PLANE_BAND).any(0)
    got_ground = _rows(ground, pc1)
    print(f"point_removal: {len(rf)} after range filter, {len(pc1)} after outlier removal, ground {got_ground.sum()} "
          f"(restatement {want_ground.sum()}, {band_p.sum()} in the plane band), points {len(points)}")
    assert np.array_equal(got_ground[~band_p], want_ground[~band_p])
    assert np.array_equal(ground, pc1[got_ground])                    # order preserved
    # the rest -> outlier removal
    rest = pc1[~got_ground]
    keep2, avg2, thr2 = ref.statistical_outlier(rest)
    band2 = np.abs(avg2 - thr2) <= OUTLIER_BAND * thr2
    got2 = _rows(points, rest)
    assert band2.sum() <= 1e-3 * len(rest) and np.array_equal(got2[~band2], keep2[~band2])
    assert np.array_equal(points, rest[got2])
    assert len(points) > 0 and len(ground) > 0


def test_point_removal_ground_vs_reference_fixture(fx, removal_run):
    """Against the reference: the Jaccard distance between the end-to-end run's ground set and the fixture's seed-0 ground set is at
    most twice the largest distance among the fixture's own three seeds (the algorithm is random; the reference's spread is
    the yardstick, factor 2 for having only three samples of it).

    The fixture's ground sets for THIS check are the reference's six my_ransac runs made where point_removal makes them: on the
    cloud after the first outlier removal (``pipe_*`` in the fixture; that step is open3d's and is the float64 restatement there).
    The runs on the range-filtered cloud (``inliers``) are a different population: the outlier removal takes 371 of the 13,648
    points away, about 85 of them within 0.15 m of the ground, and changes n, hence every sample drawn.  Against those the
    distance is 1.167e-2 with a bound of 2 * 9.89e-4 -- for the device run and for the float64 restatement of the whole pipeline
    on the CPU alike (the same figure to four digits), so that comparison says nothing about the code; it is printed below, and
    test_six_ransac_runs_on_the_fixture_cloud_follow_the_reference compares like with like on that cloud."""
    _, ground, models, rand_after = removal_run
    rf = fx["filtered"]
    keep = np.unpackbits(fx["pipe_keep"])[:len(rf)].astype(bool)
    pc1 = rf[keep]
    inl = np.unpackbits(fx["pipe_inliers"], axis=-1)[..., :len(pc1)].astype(bool)
    g = [inl[s].any(0) & (pc1[:, 2] < -1) for s in range(3)]
    spread = max(ref.jaccard_distance(g[a], g[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    got = _rows(ground, rf)
    assert not np.any(got & ~keep)                                    # nothing the first outlier removal took away
    dist = ref.jaccard_distance(got[keep], g[0])
    same = sum(models[r].tobytes() == fx["pipe_models"][0, r].tobytes() for r in range(6))
    print(f"end-to-end ground set: Jaccard distance to the reference's seed-0 ground {dist:.3e}, bound 2 * {spread:.3e}; "
          f"{same}/6 models bit-equal to the reference's; generator in step: {rand_after == fx['pipe_rand_after'][0]}")
    print(f"  (against the runs on the range-filtered cloud: {ref.jaccard_distance(got, _ground_of_runs(fx, 0)):.3e}, "
          f"bound 2 * {_reference_spread(fx):.3e})")
    assert dist <= 2 * spread


def test_trainer_with_point_removal_runs_a_step():
    from lidar4d_amd import LiDAR4D, pointprep
    from lidar4d_amd.data import SyntheticKitti360
    from lidar4d_amd.trainer import Trainer
    from oracle.detparams import fill_model
    from oracle.make_golden import SMALL_MODEL
    cfg = dict(SMALL_MODEL, density_scale=20.0, num_frames=5)
    data = SyntheticKitti360(DEV, H=32, W=256, num_frames=5, num_rays=256, seed=3)
    model = fill_model(LiDAR4D(**cfg), seed=11).to(DEV)
    random.seed(0)
    tr = Trainer(model, data, num_steps=64, chamfer=True, flow=True, init_scale=1.0, point_removal=pointprep.point_removal)
    assert sorted(tr.pc_list) == sorted(tr.pc_ground_list) == sorted(str(k) for k in range(5))
    for k in range(5):
        pc, ground = tr.pc_list[f"{k}"], tr.pc_ground_list[f"{k}"]
        print(f"frame {k}: {pc.shape[0]} non-ground, {ground.shape[0]} ground points")
        assert pc.is_cuda and pc.shape[0] > 0 and ground.shape[0] > 0 and pc.shape[1] == ground.shape[1] == 3
    torch.manual_seed(5)
    loss = float(tr.train_step(data.batch_for(2)))
    assert np.isfinite(loss)
