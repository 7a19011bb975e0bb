"""The static 3-D grid's levels evaluated inside the LDS dynamic-hash forward kernel (csrc/fused.hip dynhash_hs_fwd_lds_kernel, the
default) against the two launches it replaces (L4D_DH_HS_FUSED=0: dynhash_fwd_lds_kernel, then hashgrid_fwd_levels_kernel<3, 4, ..>).
Both write the same level-major columns with the same device function from the same fp32 coordinates, so the forward pass must agree
bit for bit; the gradients agree to the summation order of their float atomics.  Each run is a fresh process (the library reads its
switches once) with L4D_TRACE=1, whose launch log shows which of the two paths ran.

Sizes (rays x 768 samples): the smallest at which the kernel can still go wrong --
  343 rays = 263,424 samples: just above the 2^18 samples under which neither path runs; 33 chunks of 7,983 samples -- odd, and no
      multiple of 64, 1,024 or 2,048: wavefront tails, iterations without a second sample, a short last chunk;
  512 rays = 393,216 samples: chunks of exactly 8,192 samples;
  the 16-level, three-layer model: 32 tasks, and the density network is not the encode kernel's epilogue."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import hashlib, json, sys
import torch
sys.path.insert(0, %(root)r)
from lidar4d_amd import LiDAR4D
from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
from lidar4d_amd.trainer import lidar_loss
torch.manual_seed(0)
dev = "cuda"
R = %(rays)d
model = LiDAR4D(near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE, **%(model)r).to(dev)
g = torch.Generator(device=dev).manual_seed(11)
with torch.no_grad():  # visible densities and a flow that leaves the current cell
    model.hash_encoder.hash_static.params.copy_((torch.rand(model.hash_encoder.hash_static.params.shape, device=dev, generator=g) - 0.5))
    for hd in model.hash_encoder.hash_dynamic:
        for enc in hd.hash_t:
            enc.params.copy_((torch.rand(enc.params.shape, device=dev, generator=g) - 0.5))
    model.flow_net.grid_enc.params.copy_((torch.rand(model.flow_net.grid_enc.params.shape, device=dev, generator=g) - 0.5) * 2)
data = SyntheticKitti360(dev, num_rays=R, num_frames=51, seed=5)
b = data.batch_for(20)
noise = torch.rand(R, 768, device=dev, generator=g)
out = model.render(b["rays_o_lidar"], b["rays_d_lidar"], b["time"], staged=False, num_steps=768, perturb=True, noise=noise)
lidar_loss(out, b["images_lidar"]).backward()
torch.cuda.synchronize()
h = lambda t: hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
gr = model._store.flat_grad
print(json.dumps({"depth": h(out["depth_lidar"]), "image": h(out["image_lidar"]), "weights": h(out["weights"]),
                  "weights_sum": float(out["weights"].double().sum()),
                  "grad_abs_sum": float(gr.abs().double().sum()), "grad_max": float(gr.abs().max()),
                  "grad_proj": float((gr.double() * torch.linspace(-1, 1, gr.numel(), device=dev, dtype=torch.float64)).sum()),
                  "finite": bool(torch.isfinite(gr).all())}))
"""

CASES = {"default-343": (343, {}), "default-512": (512, {}), "c2-shaped-343": (343, dict(n_levels_hash=16, num_layers_sigma=3))}
FUSED, PRE_PASS = "dynhash_hs_fwd_lds_kernel", "hashgrid_fwd_levels_kernel<3, 4"


def _run(rays, model, env_extra):
    env = {k: v for k, v in os.environ.items() if k != "L4D_DH_HS_FUSED"}  # the default run is the library's default
    env.update(L4D_TRACE="1", **env_extra)
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "rays": rays, "model": model}], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]), r.stderr


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_static_levels_reproduce_the_two_launches(case):
    rays, model = CASES[case]
    got, err = _run(rays, model, {})
    ref, ref_err = _run(rays, model, {"L4D_DH_HS_FUSED": "0"})
    print(case, "fused:", got, "two launches:", ref)
    # the new code ran, and only where it should
    assert FUSED in err and PRE_PASS not in err
    assert FUSED not in ref_err and PRE_PASS in ref_err and "dynhash_fwd_lds_kernel" in ref_err
    for e in (err, ref_err):
        done = [l for l in e.splitlines() if l.startswith("[l4d] done")]
        assert done and all(l.endswith(": ok") for l in done)
    assert got["finite"] and ref["finite"] and ref["weights_sum"] > 0
    for k in ("depth", "image", "weights"):
        assert got[k] == ref[k], (case, k)  # forward: bit-identical
    for k in ("grad_abs_sum", "grad_max", "grad_proj"):  # backward: the same contributions; float atomics order the dW / plane flushes
        a, b = got[k], ref[k]
        assert abs(a - b) <= 2e-4 * max(abs(b), 1e-12) + (1e-6 * ref["grad_abs_sum"] if k == "grad_proj" else 0.0), (case, k, a, b)
