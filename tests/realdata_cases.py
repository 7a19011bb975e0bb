"""Shared by tests/test_realdata_cpu.py and tests/test_gpu_realdata.py: the fp16 train-step fixture
(tests/golden/train_step_losses_f16.npz, tools/make_golden_train_f16.py) behind tests/train_golden.py's loader, the 8 x 32
fixture sequence (oracle.detparams.write_kitti360_fixture) as KITTI360Dataset splits, and the stand-in for point_removal the
fixture's clouds were made with."""
import os

import numpy as np
import torch

import train_golden

F16_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_losses_f16.npz")
F32_CASES = train_golden.cases()
F16_CASES = [str(c) for c in np.load(F16_PATH, allow_pickle=False)["cases"]]
ALL_CASES = [("f32", t) for t in F32_CASES] + [("f16", t) for t in F16_CASES]


def load(which, tag, device="cpu"):
    """Case ``tag`` of the fp32 (``which`` = "f32") or fp16 ("f16") fixture, as train_golden.load gives it."""
    if which == "f32":
        return train_golden.load(tag, device)
    keep = train_golden.PATH
    train_golden.PATH = F16_PATH
    try:
        return train_golden.load(tag, device)
    finally:
        train_golden.PATH = keep


def pointcloud_fixture():
    """-> (keys, {key: cloud}, {key: ground cloud}, z threshold) of the reference's process_pointcloud on the fp16 fixture sequence."""
    z = np.load(F16_PATH, allow_pickle=False)
    keys = [int(k) for k in z["pointcloud__keys"]]
    return (keys, {k: z[f"pointcloud__pc_{k}"] for k in keys}, {k: z[f"pointcloud__ground_{k}"] for k in keys},
            float(z["pointcloud__ground_z"]))


def split_on_z(threshold):
    """The fixture's stand-in for point_removal: (non-ground, ground) by a split on z (metres, sensor frame)."""
    def removal(points):
        ground = points[:, 2] < threshold
        return points[~ground], points[ground]
    return removal


def fixture_dataset(root, split, device="cpu", fp16=True, num_rays=64, H=8, W=32, **kw):
    """The fixture sequence's ``split`` as a KITTI360Dataset (``root``: a directory write_kitti360_fixture has filled, or fills now)."""
    from lidar4d_amd.kitti360 import KITTI360Dataset
    from oracle.detparams import write_kitti360_fixture
    cfg = write_kitti360_fixture(str(root), H=H, W=W)  # (deterministic: writing it again changes nothing)
    return KITTI360Dataset(device=device, split=split, root_path=str(root), sequence_id=cfg["sequence_id"], scale=cfg["scale"],
                           offset=cfg["offset"], fp16=fp16, num_rays_lidar=num_rays, fov_lidar=cfg["fov_lidar"], **kw)


def evaluate_fused(c, device):
    """-> (loss, leaves) of case ``c`` with every term that has a fused node on that node (primary losses + ray chamfer, line of
    sight, patch terms); the scene-flow term replays the fixture's flow leaves through the torch restatement, as
    train_golden.evaluate does (its fused node evaluates the real flow field)."""
    from lidar4d_amd import trainer as T
    o = train_golden.opt_of(c)
    dev = torch.device(device)
    leaf = lambda k: c[k].clone().to(dev).requires_grad_(True)
    out = {"depth_lidar": leaf("depth"), "image_lidar": leaf("image"), "weights": leaf("weights"), "z_vals": c["z_vals"].to(dev)}
    images, rays_d, time = c["images"].to(dev), c["rays_d"].to(dev), c["time"].to(dev)
    data = {"images_lidar": images, "rays_d_lidar": rays_d, "time": time}
    scale, nf = float(o["scale"]), int(o["num_frames"])
    loss = T.primary_losses(out, data, scale, chamfer=True, world=1, alpha_d=o["alpha_d"], alpha_r=o["alpha_r"], alpha_i=o["alpha_i"],
                            smooth=o["smooth_factor"], depth_loss=o["depth_loss"], raydrop_loss=o["raydrop_loss"],
                            intensity_loss=o["intensity_loss"])
    model = train_golden.FixtureFlowModel(c, dev)
    if o["flow_loss"]:
        pcs = {f"{k}": c[f"pc_{k}"].to(dev).float().contiguous() for k in range(nf)}
        grounds = {f"{k}": c[f"ground_{k}"].to(dev).float().contiguous() for k in range(nf)}
        t_ground = c["flow1_t"].to(dev) if int(c["n_flow_calls"]) > 1 else None
        loss = loss + T.flow_loss(model, pcs, grounds, time, nf, t_ground=t_ground)
    gt_raydrop = images[:, :, 0]
    gt_depth = images[:, :, 2] * gt_raydrop
    if o["urf_loss"]:
        loss = loss + T.line_of_sight_loss(out, gt_depth, int(c["global_step"]), int(o["iters"]))
    loss = loss + T.patch_depth_grad_loss(out["depth_lidar"] * gt_raydrop, gt_depth, gt_raydrop, o["patch_size_lidar"], scale,
                                          alpha_grad=o["alpha_grad"], kind=o["depth_grad_loss"], sobel_grad=bool(o["sobel_grad"]),
                                          grad_loss=bool(o["grad_loss"]), grad_norm_smooth=bool(o["grad_norm_smooth"]),
                                          spatial_smooth=bool(o["spatial_smooth"]), tv_loss=bool(o["tv_loss"]),
                                          alpha_grad_norm=o["alpha_grad_norm"], alpha_spatial=o["alpha_spatial"], alpha_tv=o["alpha_tv"])
    leaves = {"g_depth": out["depth_lidar"], "g_image": out["image_lidar"], "g_weights": out["weights"]}
    for j, f in enumerate(model.flows):
        for k in ("forward", "backward"):
            leaves[f"flow{j}_{k}_grad"] = f[k]
    return loss, leaves
