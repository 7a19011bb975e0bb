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


def loss_inputs(n, half, seed=0, device="cpu"):
    """-> depth [n], image [n,2], gt [n,3] (fp16 if ``half``), rays_d [n,3], scene scale: n rays with dropped ones, exact hits, and
    depth / intensity errors on both sides of Huber's delta (0.2 * scale)."""
    from lidar4d_amd.data import KITTI360_SCALE as S
    g = torch.Generator(device=device).manual_seed(seed)
    u = lambda *s: torch.rand(*s, device=device, generator=g)
    gt = torch.stack([(u(n) > 0.25).float(), u(n), (4.0 + 60.0 * u(n)) * S], -1)
    gt = gt.half() if half else gt
    wide = (u(n) > 0.5).float()  # half of the errors well inside delta, half well beyond it
    depth = (gt[:, 2].float() + (u(n) - 0.5) * S * (0.2 + 3.8 * wide)).clamp_min(0.0)
    inten = gt[:, 1].float() + (u(n) - 0.5) * (0.2 * S + 0.5 * wide)
    depth[: n // 8] = gt[: n // 8, 2].float()
    image = torch.stack([u(n) * 1.4 - 0.2, inten], -1)
    rays_d = torch.nn.functional.normalize(u(n, 3) - 0.5, dim=-1)
    return depth.contiguous(), image.contiguous(), gt.contiguous(), rays_d.contiguous(), S


F32 = np.float32
PRIMARY_REF_N = (1, 255, 256, 257, 1000, 65793)  # 65,793 rays = 258 partials: the second stage's strided loop takes a second turn
PRIMARY_REF_SETTINGS = ((0.2, (1.0, 0.01, 0.1)), (0.1, (0.7, 0.05, 0.2)))  # (smooth, (alpha_d, alpha_r, alpha_i))


def _tree_256(red):
    """csrc/glue_dev.h block_sum_256 on every row of ``red`` [rows, 256] fp32: red[t] += red[t + s] for s = 128 ... 1."""
    red = red.copy()
    s = 128
    while s:
        red[:, :s] = red[:, :s] + red[:, s:2 * s]
        s >>= 1
    return red[:, 0]


def fixed_order_sum(values):
    """E (tests/glue_cases.py): the sum of one fp32 value per ray as the loss kernels take it (csrc/glue_dev.h).  Per workgroup of
    256 rays block_sum_256, rays past the end counting +0; then sum_partials_kernel: thread t adds partial[t], partial[t + 256],
    ... to +0 in index order, the same tree over the 256 threads, and loss = 0 + 1 * total."""
    v = np.asarray(values)
    assert v.dtype == F32 and v.ndim == 1
    pad = lambda a: np.concatenate([a, np.zeros(-a.size % 256, F32)]).reshape(-1, 256)
    acc = np.zeros(256, F32)
    for turn in pad(_tree_256(pad(v))):  # (a missing partial[t + 256 j] adds nothing in the kernel; + 0 here changes no bit: acc is never -0)
        acc = acc + turn
    return F32(0.0) + F32(1.0) * _tree_256(acc[None])[0]


def primary_losses_ref(depth, image, gt, rays_d, alpha_d, alpha_r, alpha_i, smooth, scale):
    """E (tests/glue_cases.py: numpy float32, scalars rounded to fp32 first, no contraction, IEEE division): what
    l4ds_primary_losses gives for L4DS_L1 depth, L4DS_MSE ray-drop, L4DS_MSE intensity on fp32 ground truth, every expression in the
    order step_primary_losses_kernel (csrc/stepglue.hip) writes it -> dict(loss [1], g_depth [n], g_image [n,2], pts [2,n,3],
    gt32 [n,3]).  Nothing here is computed by HIP code."""
    depth, image, gt, rays_d = (np.ascontiguousarray(a, dtype=F32) for a in (depth, image, gt, rays_d))
    alpha_d, alpha_r, alpha_i, smooth, scale = (F32(a) for a in (alpha_d, alpha_r, alpha_i, smooth, scale))
    m = gt[:, 0]
    gt_i, gt_d = gt[:, 1] * m, gt[:, 2] * m
    gs = np.minimum(np.maximum(m, smooth), F32(1.0) - smooth)
    p_r, p_i, p_d = image[:, 0], image[:, 1] * m, depth * m
    e_d, e_r, e_i = p_d - gt_d, p_r - gs, p_i - gt_i
    v_d, dv_d = np.abs(e_d), (e_d > 0).astype(F32) - (e_d < 0).astype(F32)  # L4DS_L1: |e|, and 1 / -1 / +0
    v_r, dv_r = e_r * e_r, F32(2.0) * e_r                # L4DS_MSE
    v_i, dv_i = e_i * e_i, F32(2.0) * e_i
    acc = alpha_d * v_d + alpha_r * v_r + alpha_i * v_i  # (left to right, each product rounded first)
    g_image = np.stack([alpha_r * dv_r, alpha_i * dv_i * m], -1)
    pts = np.stack([rays_d * p_d[:, None] / scale, rays_d * gt_d[:, None] / scale])
    out = dict(loss=np.array([fixed_order_sum(acc)]), g_depth=alpha_d * dv_d * m, g_image=g_image, pts=pts, gt32=gt.copy())
    assert all(a.dtype == F32 for a in out.values())
    return out


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
