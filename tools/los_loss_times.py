"""Time and peak memory of the line-of-sight loss, forward + backward, at the benchmarked shape (16,384 rays x 768 samples):
the fused node (csrc/losses.hip through lidar4d_amd.trainer.line_of_sight_loss) next to the torch restatement ``urf_loss`` on
the same tensors.  With ``--bench-parent DIR`` it also runs ``bench.py --urf`` (and ``--urf --graph``) of this tree and of the
built tree in DIR (a checkout of the parent commit) as alternating child processes, so that both sides of that comparison come
from one box.  Writes the sections of profiles/los_loss_times.txt to the path given (default: stdout).

Method of the first section: device events around one forward + backward, REPEATS of them after WARMUP, median / min / max; the
caching allocator is warm, so neither side pays for device allocations.  Peak memory: torch.cuda.max_memory_allocated over one
forward + backward minus what was allocated before it (the inputs).

    python tools/los_loss_times.py [out.txt] [--bench-parent DIR] [--bench-runs 2]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, ITERS, STEP = 16384, 768, 30000, 9000
REPEATS, WARMUP = 50, 5
BENCH_TIMEOUT_S = 400


def make_inputs(dev):
    """What the term sees in a step: sample depths on a jittered ladder, compositing weights that peak around a surface, a
    measured depth per ray (a tenth of the rays without a return)."""
    g = torch.Generator(device=dev).manual_seed(1)
    z = (torch.linspace(0.02, 0.81, T, device=dev).repeat(N, 1) + (torch.rand(N, T, device=dev, generator=g) - 0.5) * (0.79 / T))
    d = 0.05 + 0.7 * torch.rand(N, device=dev, generator=g)
    w = torch.exp(-((z - d[:, None] - 0.003) / 0.004) ** 2) * 0.3 + 1e-4 * torch.rand(N, T, device=dev, generator=g)
    d = torch.where(torch.rand(N, device=dev, generator=g) < 0.1, torch.zeros_like(d), d)
    return w.contiguous(), z.contiguous(), d.reshape(1, N).contiguous()


def fwd_bwd(fn, w, z, d):
    leaf = w.detach().requires_grad_(True)
    loss = fn({"weights": leaf, "z_vals": z}, d, STEP, ITERS)
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


def peak_mb(run):
    run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_ms(tree, extra):
    """ms/step of one ``bench.py --urf`` run of the tree (a fresh child process), or a short reason."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3", "--urf"] + extra
    try:
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=BENCH_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return None, f"timed out after {BENCH_TIMEOUT_S} s"
    if r.returncode != 0:
        return None, f"exit status {r.returncode}: {r.stderr.strip()[-200:]}"
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{") and "ms_per_step" in line:
            return float(json.loads(line)["ms_per_step"]), ""
    return None, "no result line"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--bench-parent", metavar="DIR", help="built checkout of the parent commit: run bench.py --urf there and here")
    ap.add_argument("--bench-runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken anywhere else says nothing")
    from lidar4d_amd.trainer import line_of_sight_loss, urf_loss
    out = open(args.out, "w") if args.out else sys.stdout
    say = lambda s="": print(s, file=out, flush=True)
    w, z, d = make_inputs("cuda")
    (lf, gf), (lt, gt) = fwd_bwd(line_of_sight_loss, w, z, d), fwd_bwd(urf_loss, w, z, d)
    err_l = abs(float(lf) - float(lt)) / abs(float(lt))
    err_g = float((gf - gt).abs().max() / gt.abs().max())
    f = time_ms(lambda: fwd_bwd(line_of_sight_loss, w, z, d))
    t = time_ms(lambda: fwd_bwd(urf_loss, w, z, d))
    mf, mt = peak_mb(lambda: fwd_bwd(line_of_sight_loss, w, z, d)), peak_mb(lambda: fwd_bwd(urf_loss, w, z, d))
    say(f"Line-of-sight loss, forward + backward on [{N}, {T}] weights / z_vals ({N * T * 4 / 2 ** 20:.0f} MiB each), {torch.cuda.get_device_name(0)}.")
    say(f"Device events around one forward + backward, {REPEATS} repeats after {WARMUP} warm-up; milliseconds.  Peak = device memory")
    say("allocated on top of the inputs during one forward + backward (the gradient's own 48 MiB included).")
    say()
    say("                                                     median      min      max   peak MiB")
    say(f"  line_of_sight_loss (5 launches, csrc/losses.hip)   {f[0]:8.3f} {f[1]:8.3f} {f[2]:8.3f} {mf:10.1f}")
    say(f"  urf_loss (torch ops + autograd)                    {t[0]:8.3f} {t[1]:8.3f} {t[2]:8.3f} {mt:10.1f}")
    say()
    say(f"  values: fused {float(lf):.9g}, torch {float(lt):.9g} (relative difference {err_l:.2e}); gradient difference / largest = {err_g:.2e}")
    verdict = "not slower" if f[0] <= t[0] else "SLOWER"
    say(f"  the fused node is {verdict} than urf_loss on the same tensors ({t[0] / f[0]:.2f}x by the medians)")
    if args.bench_parent:
        del w, z, d, gf, gt
        torch.cuda.empty_cache()
        say()
        say(f"bench.py --gpus 1 --steps 20 --warmup 3 --urf, ms per step, alternating child processes on this box ({args.bench_runs} runs each).")
        rows = {("parent", "eager"): [], ("this", "eager"): [], ("parent", "--graph"): [], ("this", "--graph"): []}
        for _ in range(args.bench_runs):
            for mode, extra in (("eager", []), ("--graph", ["--graph"])):
                for who, tree in (("parent", args.bench_parent), ("this", ROOT)):
                    ms, why = bench_ms(tree, extra)
                    rows[(who, mode)].append(f"{ms:.3f}" if ms is not None else f"failed ({why})")
                    print(f"bench {who} {mode}: {rows[(who, mode)][-1]}", file=sys.stderr, flush=True)
        for (who, mode), v in rows.items():
            say(f"  {who:6s} {mode:8s} {'  '.join(v)}")
        say("  (the parent's Trainer.graphs_supported() is False with urf=True: its --graph rows are eager steps)")
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
