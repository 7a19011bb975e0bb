"""The static 3-D grid's levels evaluated inside the LDS dynamic-hash forward kernel (csrc/fused.hip dynhash_hs_fwd_lds_kernel, what a
batch of 2^18 samples or more takes) against the routes a smaller batch takes: render(whole batch) == concatenation of render(pieces).
The whole batch evaluates the static grid level-major inside the LDS kernel, runs the density network as the encode kernel's epilogue
(default model) and the flow grid level-major; every piece holds at least 2^15 and fewer than 2^18 samples and takes dynhash_fwd_lds_kernel,
the static grid gathered inside the encode kernel, the network as a launch of its own and the flow grid's row kernel.  All of them
apply the same device functions to the same fp32 coordinates of a sample, and a ray's samples never meet another ray's, so the forward
pass must agree bit for bit on random tables; the gradients (``lidar_loss`` is a sum over rays) agree to the summation order of their
float atomics.  Each case is one fresh process with L4D_TRACE=1, whose launch log shows which kernels ran.

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
ro, rd, gt = b["rays_o_lidar"].reshape(1, R, 3), b["rays_d_lidar"].reshape(1, R, 3), b["images_lidar"].reshape(1, R, 3)
KEYS = ("depth_lidar", "image_lidar", "weights")
store = model._store

def run(lo, hi):  # rays [lo, hi) with their rows of noise: outputs as [rays, ...] copies, and the gradient arena of this call alone
    out = model.render(ro[:, lo:hi], rd[:, lo:hi], b["time"], staged=False, num_steps=768, perturb=True, noise=noise[lo:hi])
    lidar_loss(out, gt[:, lo:hi]).backward()
    torch.cuda.synchronize()
    res = [out[k].detach().reshape(hi - lo, -1).clone() for k in KEYS]
    grad = store.flat_grad.double().clone()
    model.zero_grad(set_to_none=False)
    return res, grad

h = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
def figures(gr):
    return {"grad_abs_sum": float(gr.abs().sum()), "grad_max": float(gr.abs().max()),
            "grad_proj": float((gr * torch.linspace(-1, 1, gr.numel(), device=dev, dtype=torch.float64)).sum()),
            "finite": bool(torch.isfinite(gr).all())}

whole, g_whole = run(0, R)
parts = [run(lo, hi) for lo, hi in %(pieces)r]
# the arena's tail behind the parameters holds the optimiser's gates (flags: "this time slice received a gradient"), not sums
g_parts = sum(p[1] for p in parts)
g_parts[store.numel:] = torch.stack([p[1][store.numel:] for p in parts]).amax(0)
cat = [torch.cat([p[0][i] for p in parts]) for i in range(len(KEYS))]
print(json.dumps({"whole": dict({k: h(t) for k, t in zip(KEYS, whole)}, weights_sum=float(whole[2].double().sum()), **figures(g_whole)),
                  "pieces": dict({k: h(t) for k, t in zip(KEYS, cat)}, **figures(g_parts)),
                  "shapes_equal": all(a.shape == c.shape for a, c in zip(whole, cat))}))
"""

# rays, the pieces' ray ranges (each 2^15 <= rays x 768 < 2^18 samples), model
CASES = {"default-343": (343, [(0, 171), (171, 343)], {}), "default-512": (512, [(0, 256), (256, 512)], {}),
         "c2-shaped-343": (343, [(0, 171), (171, 343)], dict(n_levels_hash=16, num_layers_sigma=3))}
FUSED, PRE_PASS = "dynhash_hs_fwd_lds_kernel", "hashgrid_fwd_levels_kernel<3, 4"


def _run(rays, pieces, model):
    env = dict(os.environ, L4D_TRACE="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "rays": rays, "pieces": pieces, "model": model}], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]), r.stderr


@pytest.mark.parametrize("case", sorted(CASES))
def test_whole_batch_equals_its_pieces(case):
    rays, pieces, model = CASES[case]
    assert all(2 ** 15 <= (hi - lo) * 768 < 2 ** 18 for lo, hi in pieces) and rays * 768 >= 2 ** 18
    d, err = _run(rays, pieces, model)
    got, ref = d["pieces"], d["whole"]
    print(case, "pieces:", got, "whole batch:", ref)
    # the kernel under test ran (the whole batch), the pre-pass as a launch of its own did not, and the pieces took the other LDS kernel
    assert FUSED in err and PRE_PASS not in err and "dynhash_fwd_lds_kernel" in err
    done = [l for l in err.splitlines() if l.startswith("[l4d] done")]
    assert done and all(l.endswith(": ok") for l in done)
    assert got["finite"] and ref["finite"] and ref["weights_sum"] > 0 and d["shapes_equal"]
    for k in ("depth_lidar", "image_lidar", "weights"):
        assert got[k] == ref[k], (case, k)  # forward: bit-identical
    for k in ("grad_abs_sum", "grad_max", "grad_proj"):  # backward: the same contributions; float atomics order the dW / plane flushes
        a, b = got[k], ref[k]
        assert abs(a - b) <= 2e-4 * max(abs(b), 1e-12) + (1e-6 * ref["grad_abs_sum"] if k == "grad_proj" else 0.0), (case, k, a, b)
