"""Time of one l4de_image_errors call (csrc/evalmeter.hip, through lidar4d_amd.metrics.image_errors) on the 66 x 1030 frame,
next to the same four numbers composed from stock torch ops on the device (sort-based median, avg_pool2d-based SSIM in fp64).
Writes profiles/eval_meter_times.txt's first section to the path given (default: stdout).

Method: device events around batches of BATCH back-to-back calls on one stream, REPEATS batches after a warm-up; the figure is
the median batch divided by BATCH, i.e. what a caller that enqueues evaluations back to back pays per call (launch gaps
included).  No host synchronisation inside a batch for either path.

    python tools/eval_meter_times.py [out.txt]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCH, REPEATS, WARMUP = 20, 50, 5


def torch_errors(pred, gt, lo, hi):
    """rmse, medae, ssim, psnr with the semantics of include/lidar4d_eval.h from stock torch ops (no host step either)."""
    lo_t, hi_t = pred.new_tensor(lo), pred.new_tensor(hi)
    clamp = lambda x: torch.where(x < lo_t, lo_t, torch.where(x > hi_t, hi_t, x))
    p, g = clamp(pred), clamp(gt)
    d = g - p
    mse = (d.double() ** 2).mean()
    a = d.abs().flatten().sort().values
    n = a.numel()
    med = a[n // 2] if n % 2 else (a[n // 2 - 1] + a[n // 2]) / 2
    P, G = p.double()[None, None], g.double()[None, None]
    mean = lambda x: F.avg_pool2d(x, 7, 1)
    ux, uy, uxx, uyy, uxy = mean(P), mean(G), mean(P * P), mean(G * G), mean(P * G)
    c = 49.0 / 48.0
    vx, vy, vxy = c * (uxx - ux * ux), c * (uyy - uy * uy), c * (uxy - ux * uy)
    R = G.max() - G.min()
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return torch.stack([mse.sqrt(), med.double(), S.mean(), 10 * torch.log10(float(hi) * float(hi) / mse)])


def per_call_us(fn):
    for _ in range(WARMUP):
        for _ in range(BATCH):
            fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(BATCH):
            fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1000.0 / BATCH)
    t = np.sort(np.array(times))
    return float(np.median(t)), float(t[0]), float(t[-1])


def main():
    import meters_ref as ref
    from lidar4d_amd.metrics import image_errors
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken anywhere else says nothing")
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    H, W, hi = ref.CASES["66x1030"][:3]
    pred_np, gt_np = ref.make_pair(*ref.CASES["66x1030"])
    pred, gt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(gt_np).cuda()
    want = ref.errors_f64(pred_np, gt_np, ref.LO, hi)
    a = image_errors(pred, gt, ref.LO, hi).cpu().numpy()
    b = torch_errors(pred, gt, ref.LO, hi).cpu().numpy()
    k = per_call_us(lambda: image_errors(pred, gt, ref.LO, hi))
    t = per_call_us(lambda: torch_errors(pred, gt, ref.LO, hi))
    print(f"Image error statistics of one {H} x {W} frame (rmse, medae, ssim, psnr; clamp [1e-6, {hi:g}]), {torch.cuda.get_device_name(0)}.", file=out)
    print(f"Device events around {BATCH} back-to-back calls, {REPEATS} batches after {WARMUP} warm-up batches; microseconds per call.", file=out)
    print("", file=out)
    print("                                                     median      min      max", file=out)
    print(f"  l4de_image_errors (7 launches, csrc/evalmeter.hip) {k[0]:8.1f} {k[1]:8.1f} {k[2]:8.1f}", file=out)
    print(f"  stock torch ops (sort + avg_pool2d, fp64)          {t[0]:8.1f} {t[1]:8.1f} {t[2]:8.1f}", file=out)
    print("", file=out)
    print("  values              rmse              medae             ssim              psnr", file=out)
    for name, v in (("float64 numpy  ", want), ("l4de_image_errors", a), ("stock torch ops ", b)):
        print(f"  {name:18s}" + " ".join(f"{x:17.12f}" for x in v), file=out)
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
