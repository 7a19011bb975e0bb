"""Device time of the fused MLP per hidden width -- 16, 32 and 128 through liblidar4d_mlp.so (csrc/mlp_width.hip), 64 through the
tuned kernels of liblidar4d_hip.so (csrc/mlp.hip) -- forward and backward on the SAME input rows, at the row count of the
benchmarked step (16,384 rays x 768 samples = 12,582,912 rows), for the density network's shape (in_pad 128, one hidden layer) and
the attribute networks' (in_pad 96, two hidden layers).  Writes profiles/mlp_width_kernel_times.txt to the path given (default:
stdout).

Method (that of tools/patch_grad_times.py): device events around one call (``ops.mlp_fwd`` storing the activations; ``ops.mlp_bwd``
reading them, with dx, into a zeroed grad_w), REPEATS of them after WARMUP, the widths alternating inside every repeat so that all
of them see the same box in the same minute; median / min / max.  Every buffer is allocated before the timed calls.  The yardstick
of widths 16 and 32 is the 64-wide kernel on the same rows plus 10 % (they move fewer bytes and issue fewer MFMAs; the margin
covers the box-to-box spread and the absence of tuning); width 128 is reported with its ratio only.

    python tools/mlp_width_times.py [out.txt] [--rows N]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 16384 * 768
SHAPES = [(128, 1), (96, 2)]
WIDTHS = (64, 16, 32, 128)
REPEATS, WARMUP = 20, 3
BAR = 1.10


def n_weights(hidden, in_pad, n_hidden):
    return hidden * in_pad + (n_hidden - 1) * hidden * hidden + 16 * hidden


def measure(in_pad, n_hidden, rows, dev):
    from lidar4d_amd import ops
    g = torch.Generator(device=dev).manual_seed(in_pad + n_hidden)
    x = (torch.rand(rows, in_pad, device=dev, generator=g) * 2 - 1).half()
    dy = (torch.rand(rows, 16, device=dev, generator=g) * 2 - 1).half()
    y = torch.empty(rows, 16, dtype=torch.float16, device=dev)
    dx = torch.empty(rows, in_pad, dtype=torch.float16, device=dev)
    state = {}
    for h in WIDTHS:
        w = ((torch.rand(n_weights(h, in_pad, n_hidden), device=dev, generator=g) * 2 - 1) * 0.3).half()
        state[h] = (w, torch.empty(n_hidden, rows, h, dtype=torch.float16, device=dev), torch.zeros(w.numel(), device=dev))
    times = {(h, k): [] for h in WIDTHS for k in ("fwd", "bwd")}

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    for it in range(WARMUP + REPEATS):
        for h in WIDTHS:
            w, act, gw = state[h]
            tf = timed(lambda: ops.mlp_fwd(x, w, n_hidden, save_act=True, y=y, act=act, hidden=h))
            tb = timed(lambda: ops.mlp_bwd(x, act, dy, w, n_hidden, gw, 1.0 / 128, dx=dx, hidden=h))
            if it >= WARMUP:
                times[(h, "fwd")].append(tf)
                times[(h, "bwd")].append(tb)
    assert all(bool(torch.isfinite(state[h][2]).all()) and float(state[h][2].abs().sum()) > 0 for h in WIDTHS)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--rows", type=int, default=ROWS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_width_times.py measures device time: it needs a GPU")
    lines = []
    say = lambda s="": lines.append(s)
    say(f"Fused MLP per hidden width on {torch.cuda.get_device_name(0)}: device events around one call, {args.rows:,} rows, median / min / max")
    say(f"of {REPEATS} calls after {WARMUP}, the widths alternating inside every repeat.  Width 64: csrc/mlp.hip (stored activations); the")
    say("others: csrc/mlp_width.hip.  ratio = median over the 64-wide median of the same rows; bar (widths 16, 32): ratio <= 1.10.")
    for in_pad, n_hidden in SHAPES:
        t = measure(in_pad, n_hidden, args.rows, "cuda")
        say()
        say(f"in_pad {in_pad}, n_hidden {n_hidden}")
        say("  width  pass   median ms     min     max   ratio to 64")
        for k in ("fwd", "bwd"):
            for h in sorted(WIDTHS):
                med, lo, hi = t[(h, k)]
                ratio = med / t[(64, k)][0]
                verdict = "" if h in (64, 128) else ("  within the bar" if ratio <= BAR else "  MISSES the bar")
                say(f"  {h:5d}  {k}    {med:9.3f} {lo:7.3f} {hi:7.3f}   {ratio:6.2f}{verdict}")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
