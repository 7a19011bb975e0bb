"""Write tests/golden/train_step_losses_f16.npz by running the REFERENCE's own ``Trainer.train_step`` and
``Trainer.process_pointcloud`` (model/runner.py:166-377, 924-951) on fp16 ground truth, the dtype its dataset preloads
(data/kitti360_dataset.py:141-147).

    python tools/make_golden_train_f16.py        # needs the reference checkout oracle.make_golden.REF names

The helpers are oracle/make_golden_train.py's (the scratch import of model/runner.py with stand-in modules, the seeded stub
model, the criterion table of main_lidar4d.py:183-196); nothing of the reference is copied, the fixture holds arrays only.

Two things stand in for what a CPU run lacks, and both are said here because the fixture depends on them:
  * CUDA autocast.  The reference's step runs under ``torch.cuda.amp.autocast``, whose fp32 policy casts BOTH arguments of
    l1_loss, mse_loss, huber_loss and binary_cross_entropy_with_logits to float -- without it MSELoss and HuberLoss refuse a
    half target in backward and BCE returns half.  ``AutocastFp32`` wraps every module of the criterion table (call-site
    configuration of main_lidar4d.py, not part of runner.py) and does exactly that cast.
  * ``point_removal`` (RANSAC + open3d, not installed): a deterministic split on z, ``split_on_z``, which the product's
    ``process_pointcloud(removal=...)`` is handed as well.  Everything else of process_pointcloud -- the half arithmetic of
    ``depth * mask / scale``, ``pano_to_lidar``, the transform, the keys -- is the reference's code.
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from oracle.make_golden import save  # noqa: E402
from oracle.make_golden_train import StubModel, _Chamfer, criterion_table, import_reference_trainer  # noqa: E402

SCALE = 0.010504329815187737
GROUND_Z = -1.0  # metres, sensor frame: split_on_z's threshold


class AutocastFp32(torch.nn.Module):
    """autocast's fp32 policy for a loss module: both arguments as float."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, a, b):
        return self.inner(a.float(), b.float())


def split_on_z(points):
    """(non-ground, ground) of [N, 3] points, numpy or torch: the stand-in for utils/misc.py:point_removal."""
    ground = points[:, 2] < GROUND_Z
    return points[~ground], points[ground]


def run_case(Trainer, tag, n, T, seed, frame, absent=(), near_intensity=0, **optkw):
    gen = torch.Generator().manual_seed(seed)
    opt = argparse.Namespace(patch_size_lidar=1, raydrop_loss="mse", depth_loss="l1", intensity_loss="mse", depth_grad_loss="l1",
                             smooth_factor=0.2, alpha_d=1.0, alpha_r=0.01, alpha_i=0.1, scale=SCALE, flow_loss=False, num_frames=5,
                             urf_loss=False, iters=1000, sobel_grad=False, grad_norm_smooth=False, spatial_smooth=False, tv_loss=False,
                             grad_loss=False, alpha_grad=0.1, alpha_grad_norm=0.1, alpha_spatial=0.1, alpha_tv=0.1)
    for k, v in optkw.items():
        setattr(opt, k, v)
    u = lambda *s: torch.rand(*s, generator=gen)
    images = torch.stack([(u(1, n) > 0.25).float(), u(1, n), (4.0 + 60.0 * u(1, n)) * SCALE], -1).half()  # raydrop, intensity, depth
    hit = images[0, :, 0] > 0
    assert 8 <= int(hit.sum()) <= n - 8, "rays on both sides of the mask"
    d = torch.nn.functional.normalize(u(1, n, 3) - 0.5, dim=-1)
    o = (u(1, 1, 3) - 0.5).expand(1, n, 3) * 0.01
    time = torch.tensor([[frame / (opt.num_frames - 1)]], dtype=torch.float32)
    pcs = {f"{k}": ((u(40 + 7 * k, 3) - 0.5) * 0.6).numpy() for k in range(opt.num_frames)}
    grounds = {f"{k}": ((u(11 + k, 3) - 0.5) * 0.6).numpy() for k in range(opt.num_frames)}
    for k in absent:  # a held-out frame: no clouds under its key (the fixture stores empty ones, which the product skips too)
        del pcs[f"{k}"], grounds[f"{k}"]
    gt_depth = (images[:, :, 2] * images[:, :, 0]).float()
    model = StubModel(n, T, gen, SCALE, gt_depth)
    if near_intensity:  # some predicted intensities within Huber's delta of the ground truth (the rest is far beyond it)
        with torch.no_grad():
            model.image[0, :near_intensity, 1] = images[0, :near_intensity, 1].float() + (u(near_intensity) - 0.5) * 0.2 * SCALE
    delta = 0.2 * SCALE
    for kind, err in ((opt.depth_loss, (model.depth.detach() - gt_depth)[0]), (opt.intensity_loss, (model.image.detach()[0, :, 1] - images[0, :, 1].float()))):
        if kind == "huber":
            z = err.abs()[hit]
            assert int((z < delta).sum()) >= 3 and int((z > delta).sum()) >= 3, (tag, int((z < delta).sum()), int((z > delta).sum()))

    tr = object.__new__(Trainer)
    tr.opt, tr.model, tr.cham_fn = opt, model, _Chamfer()
    tr.criterion = {k: AutocastFp32(m) for k, m in criterion_table(opt).items()}
    tr.pc_list, tr.pc_ground_list, tr.global_step, tr.device, tr.log_ptr = pcs, grounds, 250, torch.device("cpu"), None
    data = {"rays_o_lidar": o, "rays_d_lidar": d, "time": time, "images_lidar": images}
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self  # train_step moves the frame's point clouds to "the GPU"
    try:
        pred_i, gt_i, pred_d, gt_d, loss = Trainer.train_step(tr, data)
    finally:
        torch.Tensor.cuda = real_cuda
    assert loss.dtype == torch.float32
    loss.backward()
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    out = dict(n=n, T=T, frame=frame, global_step=tr.global_step, images=images, rays_o=o, rays_d=d, time=time,
               depth=model.depth.detach(), image=model.image.detach(), weights=model.weights.detach(), z_vals=model.z_vals,
               loss=loss.detach(), g_depth=z(model.depth.grad, model.depth), g_image=z(model.image.grad, model.image),
               g_weights=z(model.weights.grad, model.weights), n_flow_calls=len(model.flows))
    for k, v in vars(opt).items():
        out["opt_" + k] = np.asarray(v)
    for k in range(opt.num_frames):
        out[f"pc_{k}"] = pcs.get(f"{k}", np.zeros((0, 3), np.float32))
        out[f"ground_{k}"] = grounds.get(f"{k}", np.zeros((0, 3), np.float32))
    for j, f in enumerate(model.flows):
        out[f"flow{j}_t"] = model.flow_t[j]
        for key in ("forward", "backward"):
            out[f"flow{j}_{key}"] = f[key].detach()
            out[f"flow{j}_{key}_grad"] = z(f[key].grad, f[key])
    return {f"{tag}__{k}": v for k, v in out.items()}


CASES = (
    # tag, rays, samples, seed, frame, options
    ("default", 96, 24, 21, 2, {}),
    ("crit_huber_bce_l1", 96, 8, 22, 2, dict(depth_loss="huber", raydrop_loss="bce", intensity_loss="l1")),
    ("crit_mse_l1_huber", 96, 8, 23, 2, dict(depth_loss="mse", raydrop_loss="l1", intensity_loss="huber", alpha_d=0.7, alpha_r=0.05,
                                             alpha_i=0.2, smooth_factor=0.1, near_intensity=24)),
    ("depth_bce", 64, 8, 24, 2, dict(depth_loss="bce")),
    ("urf", 64, 48, 25, 1, dict(urf_loss=True)),
    ("patch_2x8", 96, 8, 26, 2, dict(patch_size_lidar=[2, 8], grad_loss=True)),
    ("flow_gap", 96, 16, 27, 2, dict(flow_loss=True, absent=(3,))),  # the +1 neighbour is a held-out frame
)


def run_pointcloud(Trainer):
    """The reference's process_pointcloud over its own loader of the 8 x 32 fixture sequence's ``refine`` split, fp16."""
    import data.kitti360_dataset as ref_ds
    import model.runner as ref_runner
    from oracle.detparams import write_kitti360_fixture

    root = tempfile.mkdtemp(prefix="l4d_k360_f16_")
    cfg = write_kitti360_fixture(root)
    ds = ref_ds.KITTI360Dataset(device="cpu", split="refine", root_path=root, sequence_id=cfg["sequence_id"], preload=True,
                                scale=cfg["scale"], offset=cfg["offset"], fp16=True, num_rays_lidar=16, fov_lidar=cfg["fov_lidar"])
    assert ds.images_lidar.dtype == torch.half
    tr = object.__new__(Trainer)
    tr.opt = argparse.Namespace(scale=cfg["scale"], num_frames=51)
    tr.log_ptr, tr.mute, tr.local_rank, tr.console = None, True, 0, None
    tr.log = lambda *a, **k: None
    ref_runner.point_removal = split_on_z
    tr.process_pointcloud(ds.dataloader())
    shutil.rmtree(root, ignore_errors=True)
    keys = sorted(tr.pc_list, key=int)
    assert sorted(tr.pc_ground_list, key=int) == keys
    out = {"pointcloud__keys": np.array([int(k) for k in keys]), "pointcloud__ground_z": np.float64(GROUND_Z)}
    for k in keys:
        assert len(tr.pc_list[k]) >= 8 and len(tr.pc_ground_list[k]) >= 8, "the split on z leaves points on both sides"
        out[f"pointcloud__pc_{k}"], out[f"pointcloud__ground_{k}"] = tr.pc_list[k], tr.pc_ground_list[k]
    return out


def main():
    torch.set_num_threads(4)
    Trainer, scratch = import_reference_trainer()
    arrays = {"cases": np.array([c[0] for c in CASES])}
    for tag, n, T, seed, frame, kw in CASES:
        arrays.update(run_case(Trainer, tag, n, T, seed, frame, **kw))
        print(f"{tag}: loss {float(arrays[tag + '__loss']):.6f}")
    arrays.update(run_pointcloud(Trainer))
    print("point clouds:", arrays["pointcloud__keys"].tolist(),
          [(len(arrays[f"pointcloud__pc_{k}"]), len(arrays[f"pointcloud__ground_{k}"])) for k in arrays["pointcloud__keys"]])
    save("train_step_losses_f16", **arrays)
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
