"""Ground and outlier removal for the scene-flow point clouds.  Mirror of the reference's utils/misc.py:18-154 (same function
names, argument order and meaning) on the HIP kernels of lidar4d_amd/csrc/pointprep.hip, so that ``process_pointcloud``
(runner.py:923-951) can split a REAL frame into non-ground and ground points on the device:

    point_removal = range_filter -> remove_statistical_outlier(64, 3.0) -> six my_ransac(0.15) plane fits, union,
                    z < -1 -> ground; the rest -> remove_statistical_outlier(64, 3.0) -> points

``remove_statistical_outlier`` stands for open3d's ``PointCloud.remove_statistical_outlier``.  open3d is not a dependency
and could not be run against this code: the function is written from open3d's published algorithm (mean Euclidean distance
to the ``nb_neighbors`` nearest points of the same cloud, the point itself included; keep ``v < mean + std_ratio * std`` with
the (n - 1) standard deviation) and is NOT pinned against an open3d build.  The RANSAC part is pinned against the reference's
own code (tests/golden/point_removal.npz): ``my_ransac`` consumes python's ``random`` stream exactly as the reference does,
rejected draws included, so the same seed gives the same hypotheses.  The inlier counts come from the device; a count that
differs by a point at the 0.15 m boundary (fp32 rounding of the distance) can select another, equally good plane.

Inputs are HIP tensors, outputs are HIP tensors; a CPU tensor raises ``HipExtensionError`` (no CPU fallback).  This is
start-up work: sizes of results are read back from the device, and every RANSAC batch reads back its counts.
"""
import random as _random

import numpy as np
import torch

from . import _prep_lib, ops

RANSAC_BATCH = 64  # hypotheses scored per launch (a run of my_ransac on a LiDAR frame ends after 10 to 30 accepted draws)
_MAX_REJECTED_DRAWS = 1 << 20


def _cloud(t, name):
    t = torch.as_tensor(t) if not torch.is_tensor(t) else t
    t = t.detach()
    if not t.is_cuda:
        ops._chk(t, None, name)  # raises: no CPU path
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"{name}: expected [N, >=3] points")
    return t[:, :3].to(torch.float32).contiguous()


def _u8(n, dev):
    return torch.empty(max(1, int(n)), dtype=torch.uint8, device=dev)


def range_filter(pcd, dist_min=1, dist_max=50, z_limit=(-2.5, 4)):
    """utils/misc.py:116-125: keep dist_min <= |p| <= dist_max, z_limit[0] < z < z_limit[1], not inside the ego box."""
    pts = _cloud(pcd, "pcd")
    n = pts.shape[0]
    out = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
    count = torch.zeros(1, dtype=torch.int32, device=pts.device)
    ws = _u8(_prep_lib.lib().l4dp_compact_workspace(n), pts.device)
    _prep_lib.call("l4dp_range_filter", ops._p(pts), n, float(dist_min), float(dist_max), float(z_limit[0]), float(z_limit[1]),
                   ops._p(out), None, ops._p(count), ops._p(ws), ops._stream())
    return out[: int(count.item())]


def _morton_order(pts):
    """Rows of pts sorted along a Z-order curve (10 bits per axis, one scale for the three axes) -> int32 permutation.
    Only the ORDER in which the k-nearest kernel visits the cloud: the result does not depend on it beyond fp32 summation order."""
    lo = pts.amin(dim=0)
    extent = (pts.amax(dim=0) - lo).amax().clamp_min(1e-20)
    q = ((pts - lo) * (1023.0 / extent)).nan_to_num(0.0).to(torch.int64).clamp_(0, 1023)

    def spread(v):
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        return (v | (v << 2)) & 0x09249249

    key = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    return torch.sort(key, stable=True).indices.to(torch.int32).contiguous()


def knn_mean_distance(points, nb_neighbors=64, sort=True):
    """Mean Euclidean distance of every point to its min(nb_neighbors, N) nearest points of the cloud, itself included
    -> [N] fp32.  Exact and bit-reproducible.  sort=False visits the cloud in input order (slower, same neighbours)."""
    pts = _cloud(points, "points")
    n = pts.shape[0]
    if not 1 <= int(nb_neighbors) <= _prep_lib.MAX_NEIGHBORS:
        raise ValueError(f"nb_neighbors must be in [1, {_prep_lib.MAX_NEIGHBORS}] (one neighbour per lane of a wavefront)")
    avg = torch.empty(n, dtype=torch.float32, device=pts.device)
    if n == 0:
        return avg
    order = _morton_order(pts) if sort and n > 64 else None
    ws = _u8(_prep_lib.lib().l4dp_knn_workspace(n), pts.device)
    _prep_lib.call("l4dp_knn_mean_dist", ops._p(pts), n, int(nb_neighbors), ops._p(order), ops._p(avg), ops._p(ws), ops._stream())
    return avg


def remove_statistical_outlier(points, nb_neighbors=64, std_ratio=3.0, return_stats=False):
    """open3d's ``remove_statistical_outlier`` restated (see the module docstring: unpinned) -> (kept points [M,3], their rows
    [M] int64), like open3d's (cloud, ind).  return_stats: additionally (avg [N] fp32, stats [3] fp64 = mean, std, threshold)."""
    pts = _cloud(points, "points")
    n = pts.shape[0]
    avg = knn_mean_distance(pts, nb_neighbors)
    stats = torch.zeros(3, dtype=torch.float64, device=pts.device)
    if n == 0:
        kept, ind = pts, torch.empty(0, dtype=torch.int64, device=pts.device)
    else:
        out = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
        index = torch.empty(n, dtype=torch.int32, device=pts.device)
        count = torch.zeros(1, dtype=torch.int32, device=pts.device)
        ws = _u8(_prep_lib.lib().l4dp_compact_workspace(n), pts.device)
        _prep_lib.call("l4dp_outlier_filter", ops._p(pts), ops._p(avg), n, float(std_ratio), ops._p(out), ops._p(index),
                       ops._p(count), ops._p(stats), ops._p(ws), ops._stream())
        m = int(count.item())
        kept, ind = out[:m], index[:m].to(torch.int64)
    return (kept, ind, avg, stats) if return_stats else (kept, ind)


def plane_score(points, triples, distance_threshold, y_gap=3.0):
    """Score RANSAC hypotheses on the device.  triples [H,3] integer rows of points ->
    (valid [H] int32, coeffs [H,4] fp32, counts [H] int32), all on the device (include/lidar4d_prep.h, l4dp_plane_score)."""
    pts = _cloud(points, "points")
    tri = torch.as_tensor(triples).to(device=pts.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    H = tri.shape[0]
    vc = torch.zeros(2, max(1, H), dtype=torch.int32, device=pts.device)  # valid, counts: one buffer, one read-back
    coeffs = torch.zeros(max(1, H), 4, dtype=torch.float32, device=pts.device)
    _prep_lib.call("l4dp_plane_score", ops._p(pts), pts.shape[0], ops._p(tri), H, float(y_gap), float(distance_threshold),
                   ops._p(vc[0]), ops._p(coeffs), ops._p(vc[1]), ops._stream())
    return vc[0, :H], coeffs[:H], vc[1, :H]


def plane_mask(points, coeffs, distance_threshold, mask=None):
    """mask [N] uint8 |= point within distance_threshold of any of the planes coeffs [H,4] (un-normalised)."""
    pts = _cloud(points, "points")
    co = torch.as_tensor(coeffs).to(device=pts.device, dtype=torch.float32).reshape(-1, 4).contiguous()
    if mask is None:
        mask = torch.zeros(pts.shape[0], dtype=torch.uint8, device=pts.device)
    ops._chk(mask, torch.uint8, "mask")
    _prep_lib.call("l4dp_plane_mask", ops._p(pts), pts.shape[0], ops._p(co), co.shape[0], float(distance_threshold), ops._p(mask),
                   ops._stream())
    return mask


def estimate_plane(xyz, normalize=True):
    """utils/misc.py:18-57: plane through the three points xyz [3,3] -> [4] (a, b, c, d), or None for a triple the reference
    rejects (a zero component of p1 - p0, or the three ratios (p2 - p0) / (p1 - p0) all equal)."""
    pts = _cloud(xyz, "xyz")
    if pts.shape[0] != 3:
        raise ValueError("estimate_plane: expected [3, 3]")
    valid, coeffs, _ = plane_score(pts, [[0, 1, 2]], 0.0, y_gap=0.0)
    if int(valid.item()) == 0:
        return None
    co = coeffs[0]
    if normalize:
        nrm = co[:3] / torch.sqrt((co[:3] * co[:3]).sum())
        co = torch.cat([nrm, -(nrm * pts[0]).sum().reshape(1)])
    return co


def ransac_replay(n, score, rng, P=0.99, sample_size=3, max_iterations=1000, batch=RANSAC_BATCH):
    """The sequential part of utils/misc.py:60-113 over hypotheses that are scored a batch at a time.

    ``score(triples)`` takes an int array [batch, sample_size] of drawn rows and returns (valid, counts, coeffs), each indexable by
    the position in the batch.  The loop draws ``batch`` samples ahead with ``rng.sample(range(n), sample_size)``, walks them as
    the reference's ``while i < K`` does (a rejected draw is consumed and does not count; a strictly larger count becomes the
    best model and updates K; stop at ``i >= K`` or ``i > max_iterations``) and then REWINDS ``rng`` to the draws it actually
    used, so the generator is left exactly where the reference leaves it.  -> (model = coeffs[h] of the best hypothesis, its
    sample, its count, number of draws consumed)."""
    R = range(n)
    i, K, best_count, best_model, best_sample, drawn, rejected = 0, 10, -999, None, None, 0, 0
    done = False
    while not done:
        state = rng.getstate()
        samples = [rng.sample(R, sample_size) for _ in range(batch)]
        valid, counts, coeffs = score(np.asarray(samples, dtype=np.int64))
        used = 0
        for h in range(batch):
            if not i < K:
                done = True
                break
            used += 1
            if not valid[h]:
                rejected += 1
                if rejected > _MAX_REJECTED_DRAWS and best_model is None:
                    raise RuntimeError("my_ransac: no admissible sample (the reference needs two points more than 3 m apart in y)")
                continue
            c = np.int64(counts[h])
            if c > best_count:
                best_count, best_model, best_sample = c, coeffs[h], samples[h]
                with np.errstate(divide="ignore", invalid="ignore"):
                    w = c / n
                    K = np.log(1 - P) / np.log(1.0 - np.power(w, 3))
            i += 1
            if i > max_iterations:
                done = True
                break
        drawn += used
        if used < batch:  # hand back the draws that were made ahead but not consumed
            rng.setstate(state)
            for _ in range(used):
                rng.sample(R, sample_size)
    return best_model, best_sample, int(best_count), drawn


def my_ransac(data, distance_threshold=0.3, P=0.99, sample_size=3, max_iterations=1000, rng=None):
    """utils/misc.py:60-113 -> (indices [M] int64 of the best plane's inliers, model [4] fp32: un-normalised a, b, c, d).
    rng: an object with python's ``random`` interface (sample / getstate / setstate); None = the module-level ``random``, as in
    the reference.  Hypotheses are scored on the device RANSAC_BATCH at a time; the best-so-far logic runs on the host."""
    pts = _cloud(data, "data")
    model = _ransac_model(pts, distance_threshold, P, sample_size, max_iterations, rng)
    indices = torch.nonzero(plane_mask(pts, model, distance_threshold)).flatten()
    return indices, model


def _ransac_model(pts, distance_threshold, P=0.99, sample_size=3, max_iterations=1000, rng=None):
    """my_ransac without the inlier indices: the best plane's model [4] (point_removal takes the union of six planes in one launch)."""
    if sample_size < 3:
        raise ValueError("my_ransac: sample_size must be at least 3 (a plane)")
    rng = _random if rng is None else rng

    def score(samples):
        valid, coeffs, counts = plane_score(pts, samples[:, :3], distance_threshold)
        vc = torch.stack([valid, counts]).cpu().numpy()  # the one read-back of the batch
        return vc[0], vc[1], coeffs

    model, _, _, _ = ransac_replay(pts.shape[0], score, rng, P, sample_size, max_iterations)
    return model.clone()


def point_removal(pc_raw, rng=None, return_models=False):
    """utils/misc.py:128-154: raw sensor-frame cloud [N,3] (metres) -> (non-ground points, ground points), both [*,3] fp32.
    return_models: additionally the six plane models [6,4] the split was made with."""
    pc = range_filter(pc_raw)
    pc, _ = remove_statistical_outlier(pc, 64, 3.0)
    models = torch.stack([_ransac_model(pc, 0.15, rng=rng) for _ in range(6)])
    near = plane_mask(pc, models, 0.15)                       # union of the six inlier sets
    is_ground = (near != 0) & (pc[:, 2] < -1)
    pc_ground = pc[is_ground].contiguous()
    pc_rm, _ = remove_statistical_outlier(pc[~is_ground].contiguous(), 64, 3.0)
    return (pc_rm, pc_ground, models) if return_models else (pc_rm, pc_ground)
