#!/usr/bin/env python
"""Times ``render(..., early_stop=5e-5)`` against the plain staged render on the frame and model state of ``bench.py --workload c5``
(131,072 rays, 768 samples per ray, the model as constructed under torch.manual_seed(0)) and writes profiles/early_stop_times.txt.

    python tools/early_stop_times.py [--steps 5 --warmup 2 --out profiles/early_stop_times.txt] [--bench-line FILE --parent-line FILE]

One process: the plain render and every variant are warmed up, then timed ALTERNATING (one frame of each per round) with a host clock
around work that ends in a device synchronise; the table gives each variant's median and spread over the rounds.  Per variant: the
share of the frame's samples whose density was evaluated, the number of host read-backs (one int32 per slab and ray batch but the
last slab's), peak device memory.  A second scene, the same frame with ``density_scale`` 40 (smoke()'s opaque field), shows what the
option buys where rays do end: the c5 state is a field at its random initialisation with next to no opaque surface.  Needs a GPU;
there is no fallback.  --bench-line / --parent-line: files holding bench.py's JSON line of this tree / of the parent commit, quoted
next to each other at the end of the report.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_times.txt"))
    ap.add_argument("--bench-line")
    ap.add_argument("--parent-line")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("early_stop_times.py measures on a GPU: none found")
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = LiDAR4D(near_lidar=1.0 * KITTI360_SCALE, far_lidar=81.0 * KITTI360_SCALE, num_frames=51).to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    data = SyntheticKitti360(dev, W=2048, num_rays=64 * 2048, seed=1000, frame_seed=1000)
    fr = data.frame(0)
    n_rays, T = fr["rays_o_lidar"].shape[1], 768
    reads = [0]
    item = torch.Tensor.item

    def counting_item(self):
        reads[0] += 1
        return item(self)

    def render(**kw):
        with torch.no_grad():
            return model.render(fr["rays_o_lidar"], fr["rays_d_lidar"], fr["time"], staged=True, perturb=False, num_steps=T, **kw)

    variants = [("plain", {"max_ray_batch": 4096}), ("plain", {"max_ray_batch": 16384})]
    for batch in (4096, 16384):
        for slab in (64, 96, 192):
            variants.append((f"early_stop=5e-5 slab={slab}", {"max_ray_batch": batch, "early_stop": 5e-5, "slab": slab}))
    lines = [f"early_stop_times.py: {n_rays} rays x {T} samples, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"{args.warmup} warm-up + {args.steps} timed frames per variant, alternating; host clock around render + synchronise", ""]
    for scene, scale in (("c5 state (random initialisation, density_scale 1)", 1), ("the same, density_scale 40 (opaque field)", 40.0)):
        model.density_scale = scale
        times = {i: [] for i in range(len(variants))}
        info = {}
        for rnd in range(args.warmup + args.steps):
            for i, (name, kw) in enumerate(variants):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                reads[0] = 0
                torch.Tensor.item = counting_item
                try:
                    t0 = time.perf_counter()
                    out = render(**kw)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    torch.Tensor.item = item
                if rnd >= args.warmup:
                    times[i].append(dt * 1e3)
                share = float(out["evaluated_samples"]) / (n_rays * T) if "evaluated_samples" in out else 1.0
                info[i] = (share, reads[0], torch.cuda.max_memory_allocated() / 2 ** 20, out)
        lines.append(scene)
        lines.append(f"  {'variant':34s} {'max_ray_batch':>13s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'evaluated':>10s} {'read-backs':>10s} {'peak MiB':>9s}")
        base = {}
        for i, (name, kw) in enumerate(variants):
            med = statistics.median(times[i])
            if name == "plain":
                base[kw["max_ray_batch"]] = (med, info[i][3])
            share, n_reads, peak, _ = info[i]
            lines.append(f"  {name:34s} {kw['max_ray_batch']:13d} {med:10.2f} {min(times[i]):8.2f} {max(times[i]):8.2f} {share:10.1%} {n_reads:10d} {peak:9.0f}")
        for i, (name, kw) in enumerate(variants):
            if name == "plain":
                continue
            med, ref = base[kw["max_ray_batch"]]
            out = info[i][3]
            dd = float((out["depth_lidar"] - ref["depth_lidar"]).abs().max())
            same = bool(torch.equal(out["image_lidar"], ref["image_lidar"]))
            lines.append(f"  {name} @ {kw['max_ray_batch']}: {statistics.median(times[i]) / med:.2f} x the plain render's time; max |d depth| {dd:.2e} "
                         f"(bound {5e-5 * 1.001 * float(model.far_lidar):.2e}), image equal: {same}")
        lines.append("")
    for label, path in (("bench.py default line, this tree", args.bench_line), ("bench.py default line, parent commit", args.parent_line)):
        if path and os.path.exists(path):
            found = [l.strip() for l in open(path) if l.strip().startswith("{")]
            lines.append(f"{label}: {found[-1] if found else 'no JSON line found'}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
