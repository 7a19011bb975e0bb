"""Step time and launches per step of the routes a preprocessed sequence's step can take, on the synthetic model (bench.py's
model and dataset, frame 25) with an fp16 copy of the ground truth, at 1,024 and 16,384 rays:

  new route    the batch drawn by l4ds_ray_batch (ground truth stays half), the primary losses by l4ds_primary_losses
  torch route  the batch by get_lidar_rays + gather, the primary losses by lidar_loss + ray_chamfer_loss -- what the parent
               commit does for any criterion set but l1 / mse / mse (the scene-flow term stays on its fused node on both sides)

for a non-default criterion set (huber / bce / l1) and for the default set; and the default fp32 step (SyntheticKitti360 as it
is: the same two entry points on fp32 ground truth).  Writes profiles/realdata_step_times.txt to the path given (default: stdout).

Method (that of tools/patch_grad_times.py): a host clock around STEPS eager steps that end in a device synchronise, after the loss
scale has settled; median / min / max of ROUNDS rounds, the configurations alternating.  Launches: the device kernels torch's
profiler lists for one step.

    python tools/realdata_step_times.py [out.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, ROUNDS, SETTLE, FRAME = 10, 5, 40, 25
OTHER = dict(depth_loss="huber", raydrop_loss="bce", intensity_loss="l1")


def make_dataset(n_rays, half, fused):
    from lidar4d_amd.data import SyntheticKitti360
    data = SyntheticKitti360("cuda", W=1024, num_rays=n_rays, seed=1000, frame_seed=1000)
    if half:  # the frames held in half, as KITTI360Dataset preloads them (the device draw is the one both datasets share)
        data.images = data.images.half()
    data.fused_batch = fused
    return data


def build(n_rays, half, new_route, kinds):
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE
    from lidar4d_amd.trainer import Trainer
    torch.manual_seed(0)
    model = LiDAR4D(near_lidar=1.0 * KITTI360_SCALE, far_lidar=81.0 * KITTI360_SCALE, num_frames=51).to("cuda")
    data = make_dataset(n_rays, half, new_route)
    tr = Trainer(model, data, ema_decay=0.95, **kinds)
    tr.fused_losses = new_route  # (False: lidar_loss + ray_chamfer_loss; the other terms keep their fused nodes, as in the parent)
    for _ in range(SETTLE):  # the loss scale backs off from 65536 while the gradients overflow
        tr.train_step(data.batch_for(FRAME))
    return tr


def run(tr):
    step = lambda: tr.train_step(tr.dataset.batch_for(FRAME))
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / STEPS


def launches(tr):
    from torch.profiler import ProfilerActivity, profile
    step = lambda: tr.train_step(tr.dataset.batch_for(FRAME))
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "DeviceType.CUDA" in str(e.device_type))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken anywhere else says nothing")
    out = open(args.out, "w") if args.out else sys.stdout
    say = lambda s="": print(s, file=out, flush=True)
    say(f"One eager training step of the synthetic model (bench.py's model and dataset, frame {FRAME}), {torch.cuda.get_device_name(0)}.")
    say(f"Host clock around {STEPS} steps ending in a synchronise, {ROUNDS} rounds, the configurations of a block alternating; ms per step.")
    say("Launches: device kernels torch's profiler lists for one step.")
    for n_rays in (1024, 16384):
        say()
        say(f"{n_rays} rays                                                          median      min      max   launches")
        configs = {
            "huber / bce / l1, fp16 ground truth: new route": (True, True, OTHER),
            "huber / bce / l1, fp16 ground truth: torch route": (True, False, OTHER),
            "l1 / mse / mse,  fp16 ground truth: new route": (True, True, {}),
            "l1 / mse / mse,  fp16 ground truth: torch route": (True, False, {}),
            "l1 / mse / mse,  fp32 ground truth: the default step": (False, True, {}),
        }
        trainers = {name: build(n_rays, *cfg) for name, cfg in configs.items()}
        rows = {name: [] for name in trainers}
        for _ in range(ROUNDS):
            for name, tr in trainers.items():
                rows[name].append(run(tr))
        for name, v in rows.items():
            try:
                count = str(launches(trainers[name]))
            except Exception as e:  # (a profiler that does not start must not cost the timings)
                count = f"not counted ({type(e).__name__})"
            say(f"  {name:62s} {np.median(v):8.3f} {min(v):8.3f} {max(v):8.3f}   {count}")
        del trainers
        torch.cuda.empty_cache()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
