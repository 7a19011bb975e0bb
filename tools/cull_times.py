#!/usr/bin/env python
"""Times a training step on culled samples (``Trainer(cull=1e-4, cull_slab=S)``) against the plain step on the workload and model
state of ``bench.py`` (C3: 16,384 rays x 768 samples, the model as constructed under torch.manual_seed(0), chamfer and scene-flow
terms on, eager launches) and writes profiles/cull_times.txt.

    python tools/cull_times.py [--steps 8 --warmup 3 --out profiles/cull_times.txt] [--bench-lines FILE ... --parent-lines FILE ...]
                               [--test-log FILE]

One process, one Trainer: the variants -- plain, and ``cull=1e-4`` at slabs of 64, 128 and 192 samples -- differ in the trainer's
``cull`` / ``cull_slab`` attributes alone.  All are warmed up, then timed ALTERNATING (one step of each per round) with a host clock
around ``train_step`` + a device synchronise; the table gives each variant's median and spread over the rounds, the share of the
batch's samples whose density was evaluated (mean over the timed steps) and peak device memory.  Two states: the field at its random
initialisation with density_scale 1 (nothing retires: what the march itself costs), and the same field with density_scale 40 (an
opaque field, where rays do end).  The learning rate is 0: every step does a training step's whole work and the field stays in the
state that is being measured.  Needs a GPU; there is no fallback.
--bench-lines / --parent-lines: files holding bench.py's JSON line of this tree / of the parent commit from runs taken alternately,
quoted at the end.  --test-log: the output of ``pytest -s tests/test_gpu_cull.py``, whose gradient-distance figures are quoted.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull_times.txt"))
    ap.add_argument("--bench-lines", nargs="*", default=[])
    ap.add_argument("--parent-lines", nargs="*", default=[])
    ap.add_argument("--test-log")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cull_times.py measures on a GPU: none found")
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = LiDAR4D(near_lidar=1.0 * KITTI360_SCALE, far_lidar=81.0 * KITTI360_SCALE, num_frames=51).to(dev)
    n_rays, T = 16384, 768
    data = SyntheticKitti360(dev, W=1024, num_rays=n_rays, seed=1000, frame_seed=1000)
    # lr = 0: every step is a whole training step (forward, losses, backward, loss-scale check, Adam), and the field stays in the state
    # the variant is measured on
    trainer = Trainer(model, data, lr=0.0, chamfer=True, flow=True, ema_decay=0.95, num_steps=T)
    evaluated = []
    render = model.render

    def spy(*a, **kw):
        out = render(*a, **kw)
        evaluated.append(out.get("evaluated_samples"))
        return out

    model.render = spy
    variants = [("plain", None, 128)] + [(f"cull=1e-4 slab={s}", 1e-4, s) for s in (64, 128, 192)]
    lines = [f"cull_times.py: {n_rays} rays x {T} samples per step, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"{args.warmup} warm-up + {args.steps} timed steps per variant, alternating; host clock around train_step + synchronise; eager launches, lr 0", ""]
    for scene, scale in (("random initialisation, density_scale 1 (nothing retires)", 1), ("the same field, density_scale 40 (opaque)", 40.0)):
        model.density_scale = scale
        times = {i: [] for i in range(len(variants))}
        shares = {i: [] for i in range(len(variants))}
        peak = {}
        for rnd in range(args.warmup + args.steps):
            for i, (name, eps, slab) in enumerate(variants):
                trainer.cull, trainer.cull_slab = eps, slab
                del evaluated[:]
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                trainer.train_step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rnd >= args.warmup:
                    times[i].append(dt * 1e3)
                    shares[i].append(1.0 if evaluated[0] is None else float(evaluated[0]) / (n_rays * T))
                peak[i] = torch.cuda.max_memory_allocated() / 2 ** 20
        lines.append(scene)
        lines.append(f"  {'variant':24s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'evaluated':>10s} {'peak MiB':>9s} {'x plain':>8s}")
        base = statistics.median(times[0])
        for i, (name, _, _) in enumerate(variants):
            med = statistics.median(times[i])
            lines.append(f"  {name:24s} {med:10.2f} {min(times[i]):8.2f} {max(times[i]):8.2f} {statistics.mean(shares[i]):10.1%} {peak[i]:9.0f} {med / base:8.2f}")
        lines.append("")
    trainer.cull = None
    del model.render
    for label, paths in (("bench.py, this tree", args.bench_lines), ("bench.py, parent commit", args.parent_lines)):
        for path in paths:
            if not os.path.exists(path):
                continue
            found = [l.strip() for l in open(path) if l.strip().startswith("{")]
            try:
                r = json.loads(found[-1])
                lines.append(f"{label} ({os.path.basename(path)}): {r.get('value')} {r.get('unit')}, {r.get('ms_per_step', r.get('step_ms'))} ms per step")
            except Exception:
                lines.append(f"{label} ({os.path.basename(path)}): {found[-1][:300] if found else 'no JSON line found'}")
    if args.test_log and os.path.exists(args.test_log):
        lines += ["", "tests/test_gpu_cull.py, eps = 0 (128 samples per ray, S = 64): largest per-tensor relative L2 distance of the parameter",
                  "gradients between two plain backward passes of the same inputs, and between the culled backward and the plain one",
                  "(the bound: ten times the former plus 1e-6, per tensor)"]
        lines += ["  " + l.strip() for l in open(args.test_log) if l.startswith("worst of") or l.lstrip(".F").startswith("worst of")]
        planes = [float(l.split()[-1]) for l in open(args.test_log) if "planes_encoder" in l and "plain twice" in l and "print" not in l and "(" not in l]
        if planes:
            lines += [f"  the hex-planes alone, culled against plain, over all four cases: {min(planes):.3e} .. {max(planes):.3e}"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
