"""CPU tests of the point-cloud preparation (lidar4d_amd/pointprep.py, include/lidar4d_prep.h): the numpy restatement
(tests/pointprep_ref.py) against the fixture the reference's own functions wrote, the product's host-side RANSAC replay against
the same fixture (stream consumption and the K logic, without a GPU), and the unchanged default of process_pointcloud."""
import os
import random

import numpy as np
import pytest
import torch

import pointprep_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    f = dict(np.load(os.path.join(ROOT, "tests", "golden", "point_removal.npz"), allow_pickle=False))
    f["filtered"] = f["cloud"][f["rf_index"]]
    n = int(f["n_filtered"])
    f["inliers"] = np.unpackbits(f["inliers"], axis=-1)[..., :n].astype(bool)
    return f


def test_fixture_cloud_is_reproducible(fx):
    """The cloud the GPU tests rebuild at other sizes is the generator the fixture was written with."""
    assert np.array_equal(ref.make_cloud(32, 512), fx["cloud"])


def test_restatement_equals_reference_fixture(fx):
    cloud, data = fx["cloud"], fx["filtered"]
    assert np.array_equal(np.flatnonzero(ref.range_filter_mask(cloud)), fx["rf_index"])
    assert np.array_equal(ref.range_filter(cloud), data)
    # every sample the reference drew: same verdict, bit-equal model
    for s3, ok, model in zip(fx["samples"], fx["sample_valid"], fx["sample_model"]):
        co = ref.sample_model(data, list(s3))
        assert (co is not None) == bool(ok)
        if ok:
            assert co.dtype == np.float32 and co.tobytes() == model.tobytes()
    for si, seed in enumerate(fx["seeds"]):
        rng = random.Random(int(seed))
        trace = []
        for run in range(6):
            idx, model = ref.my_ransac(data, distance_threshold=0.15, rng=rng, trace=trace)
            assert np.array_equal(idx, np.flatnonzero(fx["inliers"][si, run]))
            assert model.astype(np.float32).tobytes() == fx["models"][si, run].tobytes()
        assert np.array_equal(np.array(trace), fx["samples"][fx["sample_seed"] == si])
        assert rng.random() == fx["rand_after"][si]


@pytest.mark.parametrize("batch", [64, 5])
def test_host_replay_reproduces_reference_runs_and_generator_state(fx, batch):
    """pointprep.ransac_replay driven by a numpy fp32 scorer instead of the kernel: the six index sets, the models AND the state
    of the generator after them, for the three seeds -- with a batch larger and one smaller than a run."""
    from lidar4d_amd import pointprep
    data = fx["filtered"]
    for si, seed in enumerate(fx["seeds"]):
        rng = random.Random(int(seed))
        drawn_total = 0
        for run in range(6):
            model, sample, count, drawn = pointprep.ransac_replay(
                len(data), lambda s: ref.score_batch(data, s, 0.15), rng, batch=batch)
            want = fx["inliers"][si, run]
            assert model.tobytes() == fx["models"][si, run].tobytes()
            assert count == np.count_nonzero(want)
            assert np.array_equal(ref.plane_distance(data, model) < 0.15, want)
            assert ref.sample_model(data, sample).tobytes() == model.tobytes()
            drawn_total += drawn
        assert drawn_total == np.count_nonzero(fx["sample_seed"] == si)
        assert rng.random() == fx["rand_after"][si]


def test_host_replay_uses_module_random_like_the_reference(fx):
    from lidar4d_amd import pointprep
    data = fx["filtered"]
    random.seed(0)
    for run in range(6):
        pointprep.ransac_replay(len(data), lambda s: ref.score_batch(data, s, 0.15), random)
    assert random.random() == fx["rand_after"][0]


def test_outlier_restatement_brute_force_equals_kdtree(fx):
    data = fx["filtered"][::4]  # (brute force in float64: a quarter of the cloud keeps this quick)
    keep_b, avg_b, thr_b = ref.statistical_outlier(data, 64, 3.0, method="brute")
    assert 0 < np.count_nonzero(~keep_b) < len(data) // 10
    # n - 1 standard deviation, the point itself among its neighbours (distance 0)
    assert np.isclose(thr_b, avg_b.mean() + 3.0 * avg_b.std(ddof=1), rtol=1e-12)
    few = data[:40]
    assert np.allclose(ref.knn_mean_distance(few, 64, "brute"),
                       np.sqrt(((few[:, None].astype(np.float64) - few[None].astype(np.float64)) ** 2).sum(-1)).mean(1), rtol=1e-12)
    scipy_spatial = pytest.importorskip("scipy.spatial")
    assert scipy_spatial is not None
    keep_k, avg_k, thr_k = ref.statistical_outlier(data, 64, 3.0, method="kdtree")
    assert np.allclose(avg_b, avg_k, rtol=1e-9) and np.isclose(thr_b, thr_k, rtol=1e-9)
    assert np.array_equal(keep_b, keep_k)


def test_fixture_cloud_has_no_point_at_the_outlier_threshold(fx):
    """The GPU test's band |v - thr| <= 1e-4 thr may hold 0.1 % of the cloud; the restatement itself puts (almost) nothing there."""
    data = fx["filtered"]
    _, avg, thr = ref.statistical_outlier(data)
    assert np.count_nonzero(np.abs(avg - thr) <= 1e-4 * thr) <= 1


def test_pointprep_has_no_cpu_fallback(fx):
    from lidar4d_amd import _lib, pointprep
    pts = torch.from_numpy(fx["cloud"][:100])
    for fn in (pointprep.range_filter, pointprep.remove_statistical_outlier, pointprep.my_ransac, pointprep.point_removal,
               pointprep.knn_mean_distance):
        with pytest.raises(_lib.HipExtensionError):
            fn(pts)
    with pytest.raises(_lib.HipExtensionError):
        pointprep.estimate_plane(pts[:3])


# ---- process_pointcloud ------------------------------------------------------------------------------------------------------
class _Frames:
    """Two frames with process_pointcloud's dataset attributes (CPU tensors; convert.pano_to_lidar is stubbed below)."""
    num_frames, scale, fov = 2, 0.0125, (2.0, 26.9)

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.images = torch.rand(2, 4, 8, 3, generator=g)
        self.images[..., 0] = (self.images[..., 0] > 0.3).float()
        self.poses = torch.eye(4).repeat(2, 1, 1)
        self.poses[1, :3, 3] = torch.tensor([0.1, -0.2, 0.05])
        self.clouds = [torch.randn(50, 3, generator=g) * torch.tensor([10.0, 10.0, 1.0]) + torch.tensor([0.0, 0.0, -1.2]) for _ in range(2)]


def test_process_pointcloud_default_is_unchanged_and_removal_takes_precedence(monkeypatch):
    from lidar4d_amd import convert, trainer
    ds = _Frames()
    calls = iter(ds.clouds + ds.clouds + ds.clouds)
    monkeypatch.setattr(convert, "pano_to_lidar", lambda pano, K: next(calls))
    pc, ground = trainer.process_pointcloud(ds)
    for k in range(2):
        pts, pose = ds.clouds[k], ds.poses[k]
        is_ground = (pts[:, 2] + 1.7).abs() < 0.15          # the expression process_pointcloud has used so far
        to_world = lambda q: (q * ds.scale) @ pose[:3, :3].T + pose[:3, 3]
        assert torch.equal(pc[f"{k}"], to_world(pts[~is_ground])) and torch.equal(ground[f"{k}"], to_world(pts[is_ground]))
    # ground_split alone: as before
    pc2, ground2 = trainer.process_pointcloud(ds, ground_split=lambda p: p[:, 2] < -1.0)
    assert ground2["0"].shape[0] == int((ds.clouds[0][:, 2] < -1.0).sum())
    # removal(points) -> (non_ground, ground) wins over ground_split and may drop points
    seen = []

    def removal(p):
        seen.append(p)
        return p[:7], p[7:10]

    pc3, ground3 = trainer.process_pointcloud(ds, ground_split=lambda p: 1 / 0, removal=removal)
    assert len(seen) == 2 and pc3["1"].shape == (7, 3) and ground3["1"].shape == (3, 3)
    pose = ds.poses[1]
    assert torch.equal(ground3["1"], (ds.clouds[1][7:10] * ds.scale) @ pose[:3, :3].T + pose[:3, 3])
    import inspect
    assert inspect.signature(trainer.Trainer.__init__).parameters["point_removal"].default is None
