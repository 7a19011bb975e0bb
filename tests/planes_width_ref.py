"""Float64 restatement of the four entry points of include/lidar4d_planes.h (l4dh_planes_fwd / _bwd, l4dh_density_planes_fwd / _bwd),
written from the definition and not from the kernels: a plain gather-and-weight bilinear with border clamp (ATen grid_sampler_2d,
align_corners = True), the product over the three planes of a group, the concat over scales, the three-frame blend of
LiDAR4D.density (lidar4d.py:155-176), and the ANALYTIC adjoint of all of it -- towards the planes, the coordinates and the flow --
with no autograd.  tests/test_planes_width_cpu.py pins it against oracle/fields_ref.py before tests/test_gpu_planes_width.py lets
it judge a kernel.

One thing is taken over from fp32 on purpose: WHICH cell a coordinate falls into, and whether it counts as clipped.  A bilinear
sample is continuous across a texel centre but its derivative towards the coordinate is not, and the test shapes put samples
exactly on texel centres; there either one-sided slope is a correct answer, and the one ATen gives is the one of the cell its fp32
arithmetic selects.  So the cell index and the clip mask come from the coordinate's fp32 evaluation ``((c * 2 - 1) + 1) / 2 *
(size - 1)`` (planes_field.py:76 and ATen's unnormalise), and everything else -- the position inside the cell, the weights, the
values, the sums -- is float64 arithmetic on the fp32 inputs.  A warped coordinate ``x + flow`` is the fp32 sum, as the reference
model forms it.
"""
import numpy as np
import torch

COMBS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))  # itertools.combinations(range(4), 2): first axis -> W, second -> H
STATIC, TIME = (0, 1, 3), (2, 4, 5)
F64 = torch.float64


def time_info(t, num_frames):
    """(t0, t1, t2, has_fwd, has_bwd) of a call at time t: lidar4d.py:143,157-173 with its /num_frames quirk; fp32 values."""
    t = np.float32(t)
    f = int(t * np.float32(num_frames - 1))
    return (float(t), float(np.float32((f + 1) / num_frames)), float(np.float32((f - 1) / num_frames)), f < num_frames - 1, f > 0)


def _axis(c32, size):
    """-> (i0, i1, w0, w1, mult): lower / upper texel, their float64 weights, d(position)/d(coordinate) (0 where clipped)."""
    hi = float(size - 1)
    p32 = ((c32 * 2.0 - 1.0) + 1.0) / 2.0 * hi  # fp32: selects the cell and the clip mask (module docstring)
    inside = (p32 > 0) & (p32 < hi)
    i0 = torch.floor(p32.clamp(0.0, hi)).long()
    i1 = (i0 + 1).clamp(max=size - 1)
    c = c32.to(F64)
    p = (((c * 2.0 - 1.0) + 1.0) / 2.0 * hi).clamp(0.0, hi)
    w1 = p - i0.to(F64)
    return i0, i1, 1.0 - w1, w1, torch.where(inside, hi, 0.0).to(F64)


class _Tap:
    """One plane [1, C, H, W] sampled at (cx -> W axis, cy -> H axis): values [P, C] and what the adjoint needs."""

    def __init__(self, plane, cx, cy):
        _, C, H, W = plane.shape
        self.shape = (C, H, W)
        g = plane[0].to(F64).permute(1, 2, 0).reshape(H * W, C)
        x0, x1, wx0, wx1, self.mx = _axis(cx, W)
        y0, y1, wy0, wy1, self.my = _axis(cy, H)
        self.idx = (y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1)
        self.w = (wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1)
        self.wx0, self.wx1, self.wy0, self.wy1 = wx0, wx1, wy0, wy1
        self.v = [g[i] for i in self.idx]
        self.val = sum(w.unsqueeze(1) * v for w, v in zip(self.w, self.v))

    def adjoint(self, gv):
        """gv [P, C] = d loss / d val -> (plane gradient [1, C, H, W], d/d cx [P], d/d cy [P])."""
        C, H, W = self.shape
        gp = torch.zeros(H * W, C, dtype=F64)
        for i, w in zip(self.idx, self.w):
            gp.index_add_(0, i, w.unsqueeze(1) * gv)
        v00, v01, v10, v11 = self.v
        gx = (((v01 - v00) * self.wy0.unsqueeze(1) + (v11 - v10) * self.wy1.unsqueeze(1)) * gv).sum(1) * self.mx
        gy = (((v10 - v00) * self.wx0.unsqueeze(1) + (v11 - v01) * self.wx1.unsqueeze(1)) * gv).sum(1) * self.my
        return gp.reshape(H, W, C).permute(2, 0, 1).unsqueeze(0).contiguous(), gx, gy


class _Group:
    """The product of the three static (xy, xz, yz) or time (xt, yt, zt) planes of one scale at coords [P, 4] fp32."""

    def __init__(self, coefs, coords, time_group):
        self.cis = TIME if time_group else STATIC
        self.taps = [_Tap(coefs[ci], coords[:, COMBS[ci][0]], coords[:, COMBS[ci][1]]) for ci in self.cis]
        self.prod = self.taps[0].val * self.taps[1].val * self.taps[2].val

    def adjoint(self, gprod, grads, gcoord):
        """grads[ci] += plane gradients, gcoord [P, 4] += coordinate gradients."""
        for j, (ci, tap) in enumerate(zip(self.cis, self.taps)):
            others = [t.val for i, t in enumerate(self.taps) if i != j]
            gp, gx, gy = tap.adjoint(gprod * others[0] * others[1])
            grads[ci] += gp
            gcoord[:, COMBS[ci][0]] += gx
            gcoord[:, COMBS[ci][1]] += gy


def _zero_grads(planes):
    return [[torch.zeros(p.shape, dtype=F64) for p in coefs] for coefs in planes]


def planes_fwd(planes, xt, which=0):
    """planes: per scale the six [1, C, H, W] tensors; xt [P, 4] fp32 -> (out_s, out_d) float64 [P, n_scales * C], the one ``which``
    (1: static only, 2: time only) leaves out is None."""
    xt = xt.float()
    s = torch.cat([_Group(coefs, xt, False).prod for coefs in planes], 1) if which != 2 else None
    d = torch.cat([_Group(coefs, xt, True).prod for coefs in planes], 1) if which != 1 else None
    return s, d


def planes_bwd(planes, xt, which, dout_s, dout_d):
    """-> (plane gradients in the planes' nesting, dxt [P, 4]), float64."""
    xt = xt.float()
    C = planes[0][0].shape[1]
    grads, dxt = _zero_grads(planes), torch.zeros(xt.shape[0], 4, dtype=F64)
    for s, coefs in enumerate(planes):
        if which != 2:
            _Group(coefs, xt, False).adjoint(dout_s[:, s * C:(s + 1) * C].to(F64), grads[s], dxt)
        if which != 1:
            _Group(coefs, xt, True).adjoint(dout_d[:, s * C:(s + 1) * C].to(F64), grads[s], dxt)
    return grads, dxt


def _frames(xt, flow, tinfo):
    """The three lookups' coordinates [(coords [P, 4] fp32, present)]: (x, t0), (x + forward flow, t1), (x + backward flow, t2)."""
    t0, t1, t2, has_fwd, has_bwd = tinfo
    x, flow = xt[:, :3].float(), flow.float()
    col = lambda t: torch.full((x.shape[0], 1), t, dtype=torch.float32)
    return [(torch.cat([x, col(t0)], 1), True), (torch.cat([x + flow[:, :3], col(t1)], 1), bool(has_fwd)),
            (torch.cat([x + flow[:, 3:6], col(t2)], 1), bool(has_bwd))]


def density_fwd(planes, xt, flow, tinfo):
    """-> (plane_s, plane_d) float64: the static product at x and 0.5 d0 + 0.25 (d1 + d2), a missing neighbour replaced by d0."""
    (c0, _), (c1, has_fwd), (c2, has_bwd) = _frames(xt, flow, tinfo)
    out_s, out_d = [], []
    for coefs in planes:
        out_s.append(_Group(coefs, c0, False).prod)
        d0 = _Group(coefs, c0, True).prod
        d1 = _Group(coefs, c1, True).prod if has_fwd else d0
        d2 = _Group(coefs, c2, True).prod if has_bwd else d0
        out_d.append(0.5 * d0 + 0.25 * (d1 + d2))
    return torch.cat(out_s, 1), torch.cat(out_d, 1)


def density_bwd(planes, xt, flow, tinfo, d_out_s, d_out_d):
    """-> (plane gradients, dflow [P, 6], dxt [P, 4]), float64.  dflow: through the two warped lookups only (zero for a missing
    neighbour); dxt: d/d(xyz) through every lookup, d/d(t0) through the one at t0 (t1, t2 are constants of the call)."""
    (c0, _), (c1, has_fwd), (c2, has_bwd) = _frames(xt, flow, tinfo)
    C, P = planes[0][0].shape[1], xt.shape[0]
    grads = _zero_grads(planes)
    g0, g1, g2 = (torch.zeros(P, 4, dtype=F64) for _ in range(3))
    w0 = 0.5 + (0.0 if has_fwd else 0.25) + (0.0 if has_bwd else 0.25)
    for s, coefs in enumerate(planes):
        gs, gd = d_out_s[:, s * C:(s + 1) * C].to(F64), d_out_d[:, s * C:(s + 1) * C].to(F64)
        _Group(coefs, c0, False).adjoint(gs, grads[s], g0)
        _Group(coefs, c0, True).adjoint(w0 * gd, grads[s], g0)
        if has_fwd:
            _Group(coefs, c1, True).adjoint(0.25 * gd, grads[s], g1)
        if has_bwd:
            _Group(coefs, c2, True).adjoint(0.25 * gd, grads[s], g2)
    dflow = torch.cat([g1[:, :3], g2[:, :3]], 1)
    dxt = torch.cat([g0[:, :3] + g1[:, :3] + g2[:, :3], g0[:, 3:]], 1)
    return grads, dflow, dxt


# ---- the shapes and inputs both test files use -------------------------------------------------------------------------------
RESOLUTION = (8, 12, 16, 5)  # x, y, z, t all different: a swapped axis shows
SCALES = ((1,), (1, 2, 4))
NUM_FRAMES = 51


def fill_planes(mod, key):
    """Deterministic plane values in the ranges the model starts from (planes_field.py:48-51): static planes in [0.1, 0.5], time
    planes around their initial 1, in [0.75, 1.25] (every texel different, so that no gradient is trivially constant).
    The ranges matter to the bounds the GPU tests take over from width 8 (2e-5 relative + 1e-6): the sampler's position ``((c * 2
    - 1) + 1) / 2 * (size - 1)`` is fp32 arithmetic BY DEFINITION (ATen's), and at the finest test plane (size 64) it carries up to
    (2^-25 + 2^-24) / 2 * 63 + 2^-19 / 2 = 3.8e-6 of rounding, which reaches a sample as that times the slope between neighbouring
    texels times the other two planes' values: at most 0.4 * 0.25 (static) or 0.5 * 1.5625 (time) here, i.e. 3.8e-7 / 3.0e-6 per
    plane and axis in the worst case against a bound of 1e-6 + 2e-5 * 0.42 = 9.4e-6 for the smallest time product.  Values of
    order one and both signs (slopes up to 2.4, products through zero) would put that rounding of the DEFINITION above the bound."""
    from oracle.detparams import det_uniform
    with torch.no_grad():
        for n, p in mod.named_parameters():
            is_time = int(n.split(".")[-1]) in TIME
            p.copy_(det_uniform(tuple(p.shape), f"{key}.{n}", *((0.75, 1.25) if is_time else (0.1, 0.5))))
    return mod


def sample_inputs(P, multiscale, key="pw"):
    """xt [P, 4] and flow [P, 6], fp32: det_uniform coordinates a little beyond [0, 1], and from the front fixed rows at exactly 0
    and 1, on texel centres of every scale, at -0.25 and 1.25; the flow is large enough that some warped points leave [0, 1]."""
    from oracle.detparams import det_uniform
    xt = det_uniform((P, 4), key + ".xt", -0.05, 1.05)
    flow = det_uniform((P, 6), key + ".flow", -0.3, 0.3)
    fixed = [[0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [-0.25, 0.5, 1.25, 0.3], [1.25, -0.25, 0.5, 1.0], [0.0, 1.0, 0.5, 0.5]]
    m = max(multiscale)
    for k in (1, 3, 5):  # texel k of the finest scale along every axis (time axis: texel k % 5 of 5)
        fixed.append([k / (RESOLUTION[0] * m - 1), k / (RESOLUTION[1] * m - 1), k / (RESOLUTION[2] * m - 1), (k % 5) / (RESOLUTION[3] - 1)])
    fixed = torch.tensor(fixed, dtype=torch.float32)
    n = min(P, fixed.shape[0])
    xt[:n] = fixed[:n]
    if P > 3:
        flow[3] = 0.0  # a warped point that stays where the sample is
    return xt, flow


def n_fixed_rows():
    return 8
