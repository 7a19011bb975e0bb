"""Time and launch count of the patch depth-gradient loss, forward + backward, at the benchmarked batch (16,384 rays drawn as
1,024 patches of 2 x 8): the fused node (csrc/patchgrad.hip through lidar4d_amd.trainer.patch_depth_grad_loss) next to the torch
restatement ``depth_grad_loss`` on the same tensors; and a whole patch step of the C3 workload (bench.py's model and dataset with
``patch_size_lidar = [2, 8]``), ``Trainer.train_step`` and ``train_step_graphed``, once with ``fused_patch`` and the fused patch
draw and once with neither -- the latter is the path the parent commit takes, so both sides come from one box.  Writes
profiles/patch_grad_times.txt to the path given (default: stdout).

Method (that of tools/los_loss_times.py): device events around one forward + backward, REPEATS of them after WARMUP, median /
min / max; the caching allocator is warm.  Launches: the kernels torch's profiler lists for one forward + backward.  Steps: a host
clock around STEPS steps that end in a device synchronise, after the loss scale has settled; median / min / max of ROUNDS rounds,
the two configurations alternating.  The torch route cannot be captured (Trainer.graphs_supported): its graphed row says so.

    python tools/patch_grad_times.py [out.txt] [--no-steps]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_RAYS, PATCH = 16384, [2, 8]
REPEATS, WARMUP = 50, 5
STEPS, ROUNDS, SETTLE = 10, 3, 40


def make_inputs(dev, scale):
    """What the term sees in a patch step: depths of a smooth scene with a jump in every fifth patch, a tenth of the rays without
    a return, predictions a few millimetres off."""
    g = torch.Generator(device=dev).manual_seed(1)
    n_patch = N_RAYS // (PATCH[0] * PATCH[1])
    base = 5.0 + 35.0 * torch.rand(n_patch, 1, 1, device=dev, generator=g)
    jj = torch.arange(PATCH[1], device=dev, dtype=torch.float32).view(1, 1, -1)
    ii = torch.arange(PATCH[0], device=dev, dtype=torch.float32).view(1, -1, 1)
    metres = base + 0.0006 * jj - 0.0004 * ii
    metres[::5, :, PATCH[1] // 2:] += 0.3
    hit = (torch.rand(n_patch, *PATCH, device=dev, generator=g) > 0.1).float()
    pred_m = metres + 0.006 * (torch.rand(n_patch, *PATCH, device=dev, generator=g) - 0.5)
    flat = lambda t: t.reshape(1, -1).contiguous()
    return flat(pred_m * scale * hit), flat(metres * scale * hit), flat(hit)


def fwd_bwd(fn, pred, gt, hit, scale):
    leaf = pred.detach().requires_grad_(True)
    loss = fn(leaf, gt, hit, PATCH, scale)
    (loss * 128.0).backward()
    return loss.detach(), leaf.grad


def time_ms(run):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    t = np.sort(np.array(times))
    return float(np.median(t)), float(t[0]), float(t[-1])


def launches(run):
    from torch.profiler import ProfilerActivity, profile
    run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "DeviceType.CUDA" in str(e.device_type))


def step_times(say):
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.trainer import Trainer

    def build(fused):
        torch.manual_seed(0)
        model = LiDAR4D(near_lidar=1.0 * KITTI360_SCALE, far_lidar=81.0 * KITTI360_SCALE, num_frames=51).to("cuda")
        data = SyntheticKitti360("cuda", W=1024, num_rays=N_RAYS, seed=1000, frame_seed=1000)
        data.patch_size_lidar, data.fused_batch = PATCH, fused
        tr = Trainer(model, data, ema_decay=0.95, fused_patch=fused)
        for _ in range(SETTLE):  # the loss scale backs off from 65536 while the gradients overflow
            tr.train_step()
        return tr

    def run(tr, graphed):
        step = (lambda: tr.train_step_graphed(25)) if graphed else (lambda: tr.train_step(tr.dataset.batch_for(25)))
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / STEPS

    trainers = {"fused_patch + fused draw": build(True), "torch route (the parent's path)": build(False)}
    rows = {(name, mode): [] for name in trainers for mode in ("eager", "graphed")}
    for _ in range(ROUNDS):
        for mode in ("eager", "graphed"):
            for name, tr in trainers.items():
                if mode == "graphed" and not tr.graphs_supported():
                    continue
                rows[(name, mode)].append(run(tr, mode == "graphed"))
    say(f"One training step of the C3 workload (bench.py's model and dataset, frame 25) with patch_size_lidar = {PATCH}, ms per step:")
    say(f"host clock around {STEPS} steps ending in a synchronise, {ROUNDS} rounds, the configurations alternating.")
    say()
    say("                                                        median      min      max")
    for (name, mode), v in rows.items():
        label = f"  {name}, {mode}"
        if not v:
            say(f"{label:54s} cannot be captured (Trainer.graphs_supported() is False)")
        else:
            say(f"{label:54s} {np.median(v):8.3f} {min(v):8.3f} {max(v):8.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--no-steps", action="store_true", help="only the term, not the training steps")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken anywhere else says nothing")
    from lidar4d_amd.data import KITTI360_SCALE
    from lidar4d_amd.trainer import depth_grad_loss, patch_depth_grad_loss
    out = open(args.out, "w") if args.out else sys.stdout
    say = lambda s="": print(s, file=out, flush=True)
    pred, gt, hit = make_inputs("cuda", KITTI360_SCALE)
    (lf, gf), (lt, gt_) = fwd_bwd(patch_depth_grad_loss, pred, gt, hit, KITTI360_SCALE), fwd_bwd(depth_grad_loss, pred, gt, hit, KITTI360_SCALE)
    err_l = abs(float(lf) - float(lt)) / abs(float(lt))
    err_g = float((gf - gt_).abs().max() / gt_.abs().max())
    f = time_ms(lambda: fwd_bwd(patch_depth_grad_loss, pred, gt, hit, KITTI360_SCALE))
    t = time_ms(lambda: fwd_bwd(depth_grad_loss, pred, gt, hit, KITTI360_SCALE))
    say(f"Patch depth-gradient loss (l1, forward differences, main term), forward + backward on {N_RAYS} rays = {N_RAYS // 16} patches of "
        f"{PATCH[0]} x {PATCH[1]}, {torch.cuda.get_device_name(0)}.")
    say(f"Device events around one forward + backward (times 128, as under a loss scale), {REPEATS} repeats after {WARMUP} warm-up; milliseconds.")
    say()
    say("                                                     median      min      max")
    say(f"  patch_depth_grad_loss (csrc/patchgrad.hip)         {f[0]:8.3f} {f[1]:8.3f} {f[2]:8.3f}")
    say(f"  depth_grad_loss (torch ops + autograd)             {t[0]:8.3f} {t[1]:8.3f} {t[2]:8.3f}")
    say()
    say(f"  values: fused {float(lf):.9g}, torch {float(lt):.9g} (relative difference {err_l:.2e}); gradient difference / largest = {err_g:.2e}")
    verdict = "not slower" if f[0] <= t[0] else "SLOWER"
    say(f"  the fused node is {verdict} than depth_grad_loss on the same tensors ({t[0] / f[0]:.2f}x by the medians)")
    if not args.no_steps:
        say()
        step_times(say)
    say()
    say("Launches: device kernels torch's profiler lists for one forward + backward of the term (the multiplication by the loss scale")
    say("and its backward included on both sides).")
    try:
        nf = launches(lambda: fwd_bwd(patch_depth_grad_loss, pred, gt, hit, KITTI360_SCALE))
        nt = launches(lambda: fwd_bwd(depth_grad_loss, pred, gt, hit, KITTI360_SCALE))
        say(f"  patch_depth_grad_loss {nf}, depth_grad_loss {nt}")
    except Exception as e:  # (a profiler that does not start must not cost the timings above)
        say(f"  not counted: {type(e).__name__}: {e}")
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
