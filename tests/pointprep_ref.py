"""numpy restatement of the reference's point-cloud preparation (utils/misc.py:18-154), for tests/test_pointprep_cpu.py and
tests/test_gpu_pointprep.py.  Test infrastructure, not product code.

``range_filter`` / ``estimate_plane`` / ``my_ransac`` follow the reference's expressions operation by operation (fp32 on a
float32 cloud) and are pinned against tests/golden/point_removal.npz, which tools/make_golden_pointprep.py wrote by running the
reference's own functions.  ``knn_mean_distance`` / ``statistical_outlier`` restate open3d's ``remove_statistical_outlier`` in
float64 from its published algorithm; open3d could not be run, so that part is NOT pinned against an open3d build.
"""
import random

import numpy as np
import torch


# ---- the test clouds -----------------------------------------------------------------------------------------------------------
def make_cloud(H=32, W=512, seed=0, n_stray=300, tilt=0.03, noise_rel=0.002, noise_abs=0.02):
    """Sensor-frame cloud [N,3] fp32 of the middle frame of a SyntheticKitti360(H, W), made less tidy: seeded range noise
    (noise_rel * range + noise_abs metres, normal), n_stray stray returns, and a rotation by ``tilt`` rad about the x axis so
    that the ground is not axis-aligned."""
    from lidar4d_amd.data import SyntheticKitti360, get_lidar_rays
    ds = SyntheticKitti360("cpu", H=H, W=W, num_frames=3, num_rays=64)
    k = 1
    img = ds.images[k]
    depth = (img[..., 2] * img[..., 0]).reshape(-1).numpy().astype(np.float64) / ds.scale
    dirs = get_lidar_rays(torch.eye(4)[None], ds.fov, H, W, -1)["rays_d"][0].numpy().astype(np.float64)
    rng = np.random.default_rng(seed)
    keep = depth > 0
    r = depth[keep]
    r = r + rng.normal(size=r.shape) * (noise_rel * r + noise_abs)
    pts = dirs[keep] * r[:, None]
    stray = rng.uniform([-45, -45, -2.4], [45, 45, 3.9], size=(n_stray, 3))
    rows = rng.permutation(len(pts) + n_stray)
    pts = np.concatenate([pts, stray])[rows]          # strays scattered through the cloud, not appended
    c, s = np.cos(tilt), np.sin(tilt)
    rot = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return (pts @ rot.T).astype(np.float32)


# ---- utils/misc.py:116-125 ---------------------------------------------------------------------------------------------------
def range_filter_mask(pcd, dist_min=1, dist_max=50, z_limit=(-2.5, 4)):
    dist = np.sqrt(np.sum(pcd[:, :3] ** 2, axis=1))
    ego = (pcd[:, 0] > -2) & (pcd[:, 0] < 2) & (pcd[:, 1] > -1) & (pcd[:, 1] < 1) & (pcd[:, 2] > -2) & (pcd[:, 2] < 2)
    return (dist >= dist_min) & (dist <= dist_max) & (pcd[:, 2] > z_limit[0]) & (pcd[:, 2] < z_limit[1]) & ~ego


def range_filter(pcd, **kw):
    return pcd[range_filter_mask(pcd, **kw)]


# ---- utils/misc.py:18-57 -----------------------------------------------------------------------------------------------------
def estimate_plane(xyz, normalize=True):
    v1 = xyz[1, :] - xyz[0, :]
    v2 = xyz[2, :] - xyz[0, :]
    if not np.all(v1):
        return None
    ratio = v2 / v1
    if not ((ratio[0] != ratio[1]) or (ratio[2] != ratio[1])):
        return None
    a = (v1[1] * v2[2]) - (v1[2] * v2[1])
    b = (v1[2] * v2[0]) - (v1[0] * v2[2])
    c = (v1[0] * v2[1]) - (v1[1] * v2[0])
    if normalize:
        r = np.sqrt(a ** 2 + b ** 2 + c ** 2)
        a, b, c = a / r, b / r, c / r
    d = -(a * xyz[0, 0] + b * xyz[0, 1] + c * xyz[0, 2])
    return np.array([a, b, c, d])


def sample_model(data, s3, y_gap=3):
    """The reference's two redraw rules (utils/misc.py:83-88) -> coefficients, or None if the draw is rejected."""
    if abs(data[s3[0], 1] - data[s3[1], 1]) < y_gap:
        return None
    return estimate_plane(data[s3, :], normalize=False)


def plane_distance(data, coeffs):
    """utils/misc.py:90-91, in the arithmetic of ``data`` (fp32 like the reference on a float32 cloud, or float64)."""
    r = np.sqrt(coeffs[0] ** 2 + coeffs[1] ** 2 + coeffs[2] ** 2)
    return np.divide(np.abs(np.matmul(coeffs[:3], data.T) + coeffs[3]), r)


# ---- utils/misc.py:60-113 ----------------------------------------------------------------------------------------------------
def my_ransac(data, distance_threshold=0.3, P=0.99, sample_size=3, max_iterations=1000, rng=random, trace=None):
    """``trace``: a list that receives every drawn sample, rejected ones included."""
    max_point_num = -999
    i = 0
    K = 10
    L_data = len(data)
    R_L = range(L_data)
    while i < K:
        s3 = rng.sample(R_L, sample_size)
        if trace is not None:
            trace.append(list(s3))
        coeffs = sample_model(data, s3)
        if coeffs is None:
            continue
        d_filt = np.array(plane_distance(data, coeffs) < distance_threshold)
        near_point_num = np.sum(d_filt, axis=0)
        if near_point_num > max_point_num:
            max_point_num = near_point_num
            best_model = coeffs
            best_filt = d_filt
            w = near_point_num / L_data
            wn = np.power(w, 3)
            with np.errstate(divide="ignore", invalid="ignore"):
                K = np.log(1 - P) / np.log(1.0 - wn)
        i += 1
        if i > max_iterations:
            break
    return np.argwhere(best_filt).flatten(), best_model


def score_batch(data, samples, distance_threshold, y_gap=3):
    """What the plane-scoring kernel returns for a batch of samples, computed with the reference's fp32 expressions:
    (valid [H] int32, counts [H] int32, coeffs [H,4] fp32)."""
    H = len(samples)
    valid, counts, coeffs = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros((H, 4), np.float32)
    for h, s3 in enumerate(samples):
        co = sample_model(data, list(s3[:3]), y_gap)
        if co is None:
            continue
        valid[h], coeffs[h] = 1, co
        counts[h] = np.sum(plane_distance(data, co) < distance_threshold)
    return valid, counts, coeffs


# ---- open3d remove_statistical_outlier, from its published algorithm (float64) ----------------------------------------------------
def knn_mean_distance(points, nb_neighbors=64, method="auto"):
    """Mean Euclidean distance to the min(nb_neighbors, N) nearest points of the cloud, the point itself included -> [N] float64.
    method: "kdtree" (scipy), "brute", or "auto" (kd-tree when scipy imports)."""
    pts = np.asarray(points, dtype=np.float64)[:, :3]
    n = len(pts)
    k = min(int(nb_neighbors), n)
    if n == 0:
        return np.zeros(0)
    if method == "auto":
        try:
            import scipy.spatial  # noqa: F401
            method = "kdtree"
        except ImportError:
            method = "brute"
    if method == "kdtree":
        from scipy.spatial import cKDTree
        d, _ = cKDTree(pts).query(pts, k=k)
        return d.reshape(n, k).mean(axis=1)
    out = np.empty(n)
    for i0 in range(0, n, 256):
        diff = pts[i0:i0 + 256, None, :] - pts[None, :, :]
        d2 = np.sort(np.partition((diff * diff).sum(-1), k - 1, axis=1)[:, :k], axis=1)
        out[i0:i0 + 256] = np.sqrt(d2).mean(axis=1)
    return out


def outlier_threshold(avg, std_ratio=3.0):
    avg = np.asarray(avg, dtype=np.float64)
    mu = avg.mean()
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(((avg - mu) ** 2).sum() / (len(avg) - 1))
    return mu + std_ratio * sd


def statistical_outlier(points, nb_neighbors=64, std_ratio=3.0, method="auto"):
    """-> (keep mask [N], avg [N] float64, threshold)."""
    avg = knn_mean_distance(points, nb_neighbors, method)
    thr = outlier_threshold(avg, std_ratio)
    return avg < thr, avg, thr


def jaccard_distance(a, b):
    """1 - |a & b| / |a | b| of two boolean masks."""
    union = np.count_nonzero(a | b)
    return 0.0 if union == 0 else 1.0 - np.count_nonzero(a & b) / union
