"""Workload for profiles/planes_width_kernel_times.txt: run it under ``rocprofv3 --kernel-trace --stats -d DIR -o kt -- python
tools/planes_width_times.py MODE`` (a run of its own per mode) and summarise the database with tools/rocpd_stats.py.

P = 786,432 samples (1,024 rays x 768), the default field's planes (resolution 32^3 x 8, scales 1, 2, 4, 8), frame 25 (both
neighbours), REPS calls of everything.
  new       the four entry points of liblidar4d_planes.so for C = 4, 8, 16: l4dh_planes_fwd / _bwd (which = 0, with d/dxt),
            l4dh_density_planes_fwd / _bwd (with dflow).  Kernel names carry the width: planes_fwd_kernel<4> ...
  old-fwd   what density_features replaces at C = 8, forward only: Planes4D.forward + forward_dynamic at the two warped points
            (l4d_planes_fwd three times) and the blend in torch, under no_grad
  old       the same with autograd's backward (towards planes and flow); backward = this - old-fwd
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 6
P = 1024 * 768


def main(mode):
    from lidar4d_amd import ops
    from lidar4d_amd.planes_field import Planes4D
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    xt = torch.rand(P, 4, device=dev, generator=g)
    xt[:, 3] = 0.5
    flow = (torch.rand(P, 6, device=dev, generator=g) - 0.5) * 0.04
    tinfo = ops.time_setup(torch.tensor([0.5], device=dev), 51)
    t1, t2 = float(tinfo[1]), float(tinfo[2])
    for C in ((4, 8, 16) if mode == "new" else (8,)):
        mod = Planes4D(output_dim=C).to(dev)
        with torch.no_grad():
            for p in mod.parameters():
                p.uniform_(0.5, 1.0, generator=g)
        n_out = mod.layout.n_scales * C
        gs, gd = torch.rand(P, n_out, device=dev, generator=g), torch.rand(P, n_out, device=dev, generator=g)
        arena = mod._arena()
        for _ in range(REPS):
            if mode == "new":
                garena = torch.zeros_like(arena)
                ops.planes_fwd(mod.layout, arena, xt, 0, width_lib=True)
                ops.planes_bwd(mod.layout, arena, xt, 0, gs, gd, garena, True, width_lib=True)
                ops.density_planes_fwd(mod.layout, arena, xt, flow, tinfo)
                ops.density_planes_bwd(mod.layout, arena, xt, flow, tinfo, gs, gd, garena, want_dflow=True)
                continue
            fl = flow.clone().requires_grad_(mode == "old")
            with torch.set_grad_enabled(mode == "old"):
                x = xt[:, :3]
                ps, pd = mod(xt)
                p1 = mod.forward_dynamic(torch.cat([x + fl[:, :3], torch.full((P, 1), t1, device=dev)], -1))
                p2 = mod.forward_dynamic(torch.cat([x + fl[:, 3:], torch.full((P, 1), t2, device=dev)], -1))
                pd = 0.5 * pd + 0.25 * (p1 + p2)
                if mode == "old":
                    torch.autograd.backward([ps, pd], [gs, gd])
        torch.cuda.synchronize()
    print(f"planes_width_times {mode}: {REPS} repetitions of P = {P}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "new")
