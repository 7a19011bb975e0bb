"""Inputs for the tests of the patch depth-gradient loss (tests/test_patchgrad_cpu.py, tests/test_gpu_patchgrad.py): the
smallest shapes at which csrc/patchgrad.hip can still go wrong, built so that every decision the term takes is taken both ways.

Per patch the ground truth (metres) is a smooth ramp, |slope| at most 0.8 mm per pixel: forward differences stay below 1 mm
and interior Sobel responses below 6.4 mm, clear of the 10 mm threshold.  At a deterministic subset of the x pairs a jump of
5 cm and more is planted (everything right of the pair in that row is lifted), far on the other side.  ``hit`` drops roughly
a fifth of the pixels; a dropped pixel reads 0 in the masked depths, which breaks the smoothness of every pair it is part of.
Predictions are the ground truth plus a per-patch offset and noise of +-3 mm per pixel, so that |a - b| falls on both sides
of the Huber delta (0.2 * scale: 2.1 mm at the KITTI-360 scale, 3.1 mm at 2^-6).

Every depth in metres is a multiple of 2^-12 m below 64 m.  With ``scale`` a power of two (SCALE_POW2) the scaled values and all
sums of a few of them are exact in fp32, so a 3 x 3 stencil gives the same bits in whatever order a convolution library adds
its taps: the Sobel cases use it.  The forward-difference cases use the KITTI-360 scale, where the scaling itself rounds.

``6x2x8`` additionally plants: patch 1 with every pixel dropped; patch 2 with pred == gt exactly on a ramp that falls along x
(a == b there: ties, gradient 0); patch 3 with a perfectly flat prediction (``flat=False`` leaves it out: with the cosine
criterion torch's own gradient there is of order 1e8 and nothing meaningful can be compared)."""
import torch

KITTI360_SCALE = 0.010504329815187737
SCALE_POW2 = 2.0 ** -6

# name -> (number of patches, patch_size as the dataset attribute holds it)
CASES = {
    "1x2x2": (1, [2, 2]),       # minimum patch, one difference per row
    "6x2x8": (6, [2, 8]),       # the reference's default, with plants
    "8x3x3": (8, 3),            # odd size, patches straddle a wavefront
    "4x4x8": (4, [4, 8]),       # half-wavefront patches
    "3x8x16": (3, [8, 16]),     # a patch larger than one wavefront
    "300x2x8": (300, [2, 8]),   # more than one workgroup: partials, striding
    "1x32x32": (1, [32, 32]),   # the size limit
}
MULTI_PATCH = [name for name, (n, _) in CASES.items() if n > 1]
# Past the bounded grids of csrc/patchgrad.hip (PG_THREADS 256, PG_WAVES 4, PG_MAX_BLOCKS 1024): the device tests only, the CPU tests
# iterate CASES.
# Their pixels are dropped at 3 % instead of a fifth and every 29th x pair jumps instead of every fifth: among a thousand patches
# and more, the denser plants leave some patch with one or two masked-in Sobel pixels whose prediction response is exactly 0 on the
# lattice, where the cosine criterion is singular (as on the FLAT patch below: torch's own gradient is of order 1e9 there and sets
# a scale against which nothing else can be compared).  Every decision is still taken both ways, in every patch.
STRIDE_DROP, STRIDE_JUMP_EVERY = 0.03, 29
STRIDE_CASES = {
    "4101x8x8": (4101, [8, 8]),    # 64 pixels: per_wave 1, 4 patches a group, 1026 groups -> `group += gridDim.x` and the
                                   # __syncthreads() between two groups of one workgroup; 262,464 elements -> pg_scale_kernel strides
    "1030x5x13": (1030, [5, 13]),  # 65 pixels: BIG, a patch a group, strided; not a multiple of 256
    "9x5x7": (9, [5, 7]),          # 35 pixels: per_wave 1 with 29 idle lanes a wavefront; the third group holds one patch
}
ALL_DROPPED, EXACT, FLAT = 1, 2, 3  # the planted patches of 6x2x8
KINDS = ("l1", "mse", "huber", "cos")


def shape_of(name):
    n, patch = (CASES.get(name) or STRIDE_CASES[name])
    px, py = (patch, patch) if isinstance(patch, int) else patch
    return n, px, py


def make(name, scale=KITTI360_SCALE, flat=True, half=False, seed=0):
    """-> dict(pred, gt, hit [1, n] in ray order, depths masked by hit as Trainer.compute_loss hands them over; patch_size; scale;
    n_patch, px, py).  fp32 on the CPU; half=True: gt and hit as fp16 (what KITTI360Dataset preloads)."""
    n, px, py = shape_of(name)
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, name)))
    grid = lambda t: torch.round(t * 4096.0) / 4096.0
    ii = torch.arange(px, dtype=torch.float32).view(1, px, 1)
    jj = torch.arange(py, dtype=torch.float32).view(1, 1, py)
    base = 5.0 + 35.0 * torch.rand(n, 1, 1, generator=g)
    slope = lambda: (0.0002 + 0.0006 * torch.rand(n, 1, 1, generator=g)) * torch.where(torch.rand(n, 1, 1, generator=g) < 0.5, -1.0, 1.0)
    sx, sy = slope(), slope()
    if name == "6x2x8":
        sx[EXACT] = -sx[EXACT].abs()  # falls along x: q(i,j) - q(i,j+1) > 0, so |pgx| == ggx where pred == gt
    metres = base + sx * jj + sy * ii
    # jumps: every fifth x pair (counted over the whole case, rows included) lifts the rest of its row by 5 cm ... 45 cm
    pair = torch.arange(n * px * (py - 1)).view(n, px, py - 1)
    jump = torch.where(pair % (5 if name in CASES else STRIDE_JUMP_EVERY) == 2, 0.05 + 0.1 * (pair % 4).float(), torch.zeros(()))
    if name == "6x2x8":
        jump[EXACT] = 0.0
    metres[:, :, 1:] += torch.cumsum(jump, dim=2)
    metres = grid(metres)
    hit = (torch.rand(n, px, py, generator=g) > (0.2 if name in CASES else STRIDE_DROP)).float()
    pred_m = grid(metres + 0.02 * (torch.rand(n, 1, 1, generator=g) - 0.5) + 0.006 * (torch.rand(n, px, py, generator=g) - 0.5))
    if name == "6x2x8":
        hit[ALL_DROPPED] = 0.0
        hit[EXACT] = 1.0
        pred_m[EXACT] = metres[EXACT]
        if flat:
            pred_m[FLAT] = 12.5
    gt = (metres * scale) * hit      # scene units, masked by the ray-drop
    pred = (pred_m * scale) * hit
    if half:
        gt, hit = gt.half(), hit.half()
    _, patch = (CASES.get(name) or STRIDE_CASES[name])
    return {"pred": pred.reshape(1, -1).contiguous(), "gt": gt.reshape(1, -1).contiguous(), "hit": hit.reshape(1, -1).contiguous(),
            "patch_size": patch, "scale": scale, "n_patch": n, "px": px, "py": py}


def run(fn, c, device=None, upstream=1.0, **kw):
    """-> (loss [0-dim], d (loss * upstream) / d pred) of ``fn`` (depth_grad_loss or patch_depth_grad_loss) on case ``c``."""
    to = (lambda t: t.to(device)) if device is not None else (lambda t: t)
    leaf = to(c["pred"]).clone().requires_grad_(True)
    loss = fn(leaf, to(c["gt"]), to(c["hit"]), c["patch_size"], c["scale"], **kw)
    (g,) = torch.autograd.grad(loss * upstream, leaf, allow_unused=True)
    return loss.detach(), (torch.zeros_like(leaf) if g is None else g)


def mask_of(c, sobel=False):
    """The main term's mask [n_patch, px, py - 1] (forward differences) or [n_patch, px, py] (Sobel), as the restatement forms it."""
    from lidar4d_amd.trainer import _patch_grads
    n, px, py = c["n_patch"], c["px"], c["py"]
    q = (c["gt"].float().reshape(n, 1, px, py) / c["scale"])
    hit = c["hit"].float().reshape(n, 1, px, py)
    ggx, _ = _patch_grads(q, sobel)
    return ((hit if sobel else hit[:, :, :, :-1]) * (ggx.abs() < 0.01).float()).reshape(n, px, -1)
