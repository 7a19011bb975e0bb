#!/usr/bin/env python
"""Times one C5-sized novel-view frame (64 x 2048 rays x 768 samples, staged in chunks of 4096 rays) rendered without a gradient
three ways and writes profiles/occupancy_times.txt:

    early_stop alone                      this tree, and the parent commit (--rows-out there, --parent-rows here)
    early_stop + occupancy                this tree: OccupancyGrid.build per frame, then the march that skips

    python tools/occupancy_times.py [--frames 5 --warmup 2 --out profiles/occupancy_times.txt] [--rows-out FILE] [--parent-rows FILE]

Two fields, both the default model as constructed under torch.manual_seed(0).  "surface": row 0 of the density network's output
matrix times -60 -- the gain that gives the early-stop tests' mixed scene its contrast, sigma spans several e-folds along a ray --
and a density_scale chosen here so that a sample at the 70th percentile of sigma (over 2^16 points of the box) has a per-sample
optical depth of 1: a field of high contrast whose dense part is opaque (the hash grids vary below the size of a grid cell,
though: as measured, every ray ends within its first slab and every cell holds a dense probe).  "random initialisation": the field
as constructed, density_scale 1: sigma is nearly uniform, the built grid is full, and the option can only cost its build and flags.
The variants of a field are warmed up, then timed ALTERNATING (one frame of each per round) with a host clock around the call and
a device synchronise; the table gives the median and spread of the frame time (the grid's build included), the build alone, and
the share of the frame's samples that were evaluated.  A third variant marches through a hand-made grid, a shell of cells between 0.3
and 0.6 of the box's half width, which is not the field's: what the march costs when it does skip.  The file written by --rows-out holds the early_stop-alone rows of the tree
it ran in (run this same file from a checkout of the parent commit; it needs nothing of lidar4d_amd.occupancy there).
No speed-up is promised: this is the measurement.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=ROOT, help="the tree whose lidar4d_amd is measured (default: the one this file is in)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows-out")
    ap.add_argument("--parent-rows")
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--slab", type=int, default=96)
    ap.add_argument("--resolution", type=int, default=128)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("occupancy_times.py measures on a GPU: none found")
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    try:
        from lidar4d_amd.occupancy import OccupancyGrid
    except ImportError:
        OccupancyGrid = None  # the parent commit: early_stop alone
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = LiDAR4D(near_lidar=1.0 * KITTI360_SCALE, far_lidar=81.0 * KITTI360_SCALE, num_frames=51).to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    H, W, T = 64, 2048, 768
    data = SyntheticKitti360(dev, H=H, num_rays=4096, seed=1000, frame_seed=1000)
    fr = data.frame(25, W=W)
    ro, rd, t = fr["rays_o_lidar"], fr["rays_d_lidar"], fr["time"]
    n = ro.shape[1]
    sample_dist = float((np.float32(model.far_lidar) - np.float32(model.near_lidar)) / np.float32(T))
    sn = model.sigma_net
    row0 = slice(sn.params.numel() - 16 * sn.n_neurons, sn.params.numel() - 15 * sn.n_neurons)
    kw = dict(staged=True, max_ray_batch=4096, num_steps=T, perturb=False, early_stop=args.eps, slab=args.slab)

    def plain():
        return model.render(ro, rd, t, **kw), 0.0

    def skipping():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid = OccupancyGrid.build(model, t, num_steps=T, resolution=args.resolution)
        torch.cuda.synchronize()
        build = time.perf_counter() - t0
        skipping.share = float(grid.mask().float().mean())
        return model.render(ro, rd, t, occupancy=grid, **kw), build * 1e3

    def shell():
        # NOT the field's grid: the cells between 0.3 and 0.6 of the box's half width around its middle.  What the march costs when it
        # does skip; the picture it renders is the field's inside that shell only.
        if shell.grid is None:
            c = (torch.arange(args.resolution, device=dev) + 0.5) / args.resolution * 2 - 1
            r = (c.view(-1, 1, 1) ** 2 + c.view(1, -1, 1) ** 2 + c.view(1, 1, -1) ** 2).sqrt()
            shell.grid = OccupancyGrid.from_mask((r >= 0.3) & (r <= 0.6), model.bound)
        return model.render(ro, rd, t, occupancy=shell.grid, **kw), 0.0

    shell.grid = None
    variants = [("early_stop alone", plain)]
    if OccupancyGrid is not None:
        variants += [("early_stop + occupancy", skipping), ("early_stop + a hand-made shell", shell)]
    head = [f"occupancy_times.py: one frame of {H} x {W} = {n} rays x {T} samples, staged in chunks of 4096 rays, no gradient; "
            f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
            f"early_stop={args.eps:g}, slab={args.slab}; grid: resolution {args.resolution}, probes 2, min_depth 1e-3 (the unmeasured default), dilate 1",
            f"{args.warmup} warm-up + {args.frames} timed frames per variant, alternating; host clock around build + render + synchronise", ""]
    lines, rows = [], {}
    for scene in ("surface", "random initialisation"):
        if scene == "surface":
            with torch.no_grad():
                sn.params[row0] *= -60.0
                pts = torch.rand(1 << 16, 3, device=dev) * 2 * model.bound - model.bound
                sigma = model.density(pts, t)["sigma"].float()
                q = float(torch.quantile(sigma, 0.7))
            model.density_scale = 1.0 / (q * sample_dist)
            note = f"surface: density row x -60, density_scale {model.density_scale:.3e} (optical depth 1 per sample at the 70th percentile of sigma)"
        else:
            with torch.no_grad():
                sn.params[row0] /= -60.0
            model.density_scale = 1.0
            note = "random initialisation: the field as constructed, density_scale 1"
        times, builds, shares = {}, {}, {}
        with torch.no_grad():
            for rnd in range(args.warmup + args.frames):
                for name, fn in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out, build_ms = fn()
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rnd >= args.warmup:
                        times.setdefault(name, []).append(dt)
                        builds.setdefault(name, []).append(build_ms)
                        shares[name] = int(out["evaluated_samples"])
        lines.append(note)
        lines.append(f"  {'variant':44s} {'frame ms':>9s} {'min':>8s} {'max':>8s} {'build ms':>9s} {'evaluated_samples':>18s} {'share':>7s}")
        for name, _ in variants:
            rows[f"{scene}: {name}"] = dict(ms=times[name], build_ms=builds[name], evaluated=shares[name])
        table = [(name + ", this tree", rows[f"{scene}: {name}"]) for name, _ in variants]
        if args.parent_rows and os.path.exists(args.parent_rows):
            parent = json.load(open(args.parent_rows))
            key = f"{scene}: early_stop alone"
            if key in parent:
                table.insert(1, ("early_stop alone, parent commit", parent[key]))
        for name, r in table:
            lines.append(f"  {name:44s} {statistics.median(r['ms']):9.2f} {min(r['ms']):8.2f} {max(r['ms']):8.2f} {statistics.median(r['build_ms']):9.2f} "
                         f"{r['evaluated']:18d} {r['evaluated'] / (n * T):7.1%}")
        if OccupancyGrid is not None:
            lines.append(f"  (cells set in the built grid: {skipping.share:.1%})")
        lines.append("")
    text = "\n".join(head + lines)
    print(text)
    if args.rows_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.rows_out)), exist_ok=True)
        json.dump(rows, open(args.rows_out, "w"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
