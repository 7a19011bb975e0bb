"""GPU tests of empty-space skipping (``render(..., early_stop=eps, slab=S, occupancy=grid)``: the slab flags of ``l4d_sample_rays``
in csrc/render.hip, lidar4d_amd/occupancy.py, ``early_stop.run_skipping``) against the numpy restatement of tests/occupancy_ref.py --
pinned on the CPU by tests/test_occupancy_cpu.py -- and against the march without a grid.  Run with ``-m gpu`` on an MI355X.

Flag shapes: 1, 3 and 65 rays (one wavefront, one workgroup of four with an idle wavefront, seventeen workgroups with a tail); 1, 63, 64
and 130 samples; slabs of 1, 7, 64 and 1000 (below, at and above a wavefront's stride, longer than the ray); grids of 1, 5 and 33
cells a side (33^3 is no multiple of 32)."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import early_stop_ref as er
import occupancy_ref as oref
from test_early_stop_cpu import G, MIXED_SCALE, OPAQUE_SCALE, RAY_SEED, TIME, build_scene
from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR, FAR, BOUND = SMALL_MODEL["near_lidar"], SMALL_MODEL["far_lidar"], 1
N_RAYS, T_STEPS, SLAB = 37, 130, 32
KEYS = ("depth_lidar", "image_lidar", "weights_sum_lidar", "weights", "z_vals", "mask_count", "retired_at", "evaluated_samples")


def _mask_list(out):
    return torch.sort(out["mask_idx"][:int(out["mask_count"])]).values


# ---- 1. the flags kernel -------------------------------------------------------------------------------------------------------
def _flag_rays(N):
    """[N, 3] origins and directions: ray 0 starts outside the box (every clipped position sits on u = 1, the R - 1 clamp), ray 1
    runs along the x axis, the rest are the early-stop tests' rays with their origins spread over the box."""
    ro, rd = make_rays(N, 11)
    ro, rd = ro.view(-1, 3).clone(), rd.view(-1, 3).clone()
    ro += torch.linspace(-0.9, 0.9, N).unsqueeze(1)
    ro[0], rd[0] = torch.tensor([3.0, 3.0, 3.0]), torch.tensor([1.0, 1.0, 1.0]) / 3 ** 0.5
    if N > 1:
        ro[1], rd[1] = torch.tensor([-0.9, 0.1, -0.3]), torch.tensor([1.0, 0.0, 0.0])
    return ro.contiguous(), rd.contiguous()


def _flag_masks(R):
    rng = np.random.default_rng(100 + R)
    corner = np.zeros((R, R, R), bool)
    corner[R - 1, R - 1, R - 1] = True
    return {"random": rng.random((R, R, R)) < 0.5, "set": np.ones((R, R, R), bool), "clear": np.zeros((R, R, R), bool), "corner": corner}


@pytest.mark.parametrize("T", [1, 63, 64, 130])
@pytest.mark.parametrize("N", [1, 3, 65])
def test_slab_flags_are_the_reference_bits(N, T):
    from lidar4d_amd import ops
    from lidar4d_amd.occupancy import OccupancyGrid
    ro, rd = _flag_rays(N)
    lin = torch.linspace(0.0, 1.0, T, device=DEV)
    ro_d, rd_d = ro.to(DEV), rd.to(DEV)
    z0, xyz0 = ops.sample_rays(ro_d, rd_d, lin, None, NEAR, FAR, BOUND)
    noise = torch.rand(N, T, generator=torch.Generator().manual_seed(N * T)).to(DEV)
    zn, _ = ops.sample_rays(ro_d, rd_d, lin, noise, NEAR, FAR, BOUND, want_xyz=False)
    lin_h = lin.cpu().numpy()
    seen = set()
    for R in (1, 5, 33):
        for name, m in _flag_masks(R).items():
            grid = OccupancyGrid.from_mask(torch.from_numpy(m).to(DEV), BOUND)
            assert grid.bits.is_cuda and np.array_equal(grid.bits.cpu().numpy(), oref.pack(m))
            for slab in (1, 7, 64, 1000):
                z, xyz, flags = ops.sample_rays(ro_d, rd_d, lin, None, NEAR, FAR, BOUND, occ=(grid.bits, R), slab=slab)
                z_ref, want = oref.slab_flags(m, ro.numpy(), rd.numpy(), lin_h, NEAR, FAR, BOUND, slab)
                assert flags.dtype == torch.uint8 and flags.shape == (N, -(-T // slab))
                assert torch.equal(flags.cpu(), torch.from_numpy(want)), (R, name, slab)
                assert torch.equal(z, z0) and torch.equal(xyz, xyz0) and np.array_equal(z.cpu().numpy(), z_ref), (R, name, slab)
                seen.update(want.reshape(-1).tolist())
                if name == "corner":
                    assert bool(flags[0].all())  # the ray outside the box: every sample in the last cell
            # without xyz, and with jitter (the reference reads the device's depths, which the call without a grid pins)
            z, none, flags = ops.sample_rays(ro_d, rd_d, lin, noise, NEAR, FAR, BOUND, want_xyz=False, occ=(grid.bits, R), slab=7)
            _, want = oref.slab_flags(m, ro.numpy(), rd.numpy(), None, None, None, BOUND, 7, z_vals=zn.cpu().numpy())
            assert none is None and torch.equal(z, zn) and torch.equal(flags.cpu(), torch.from_numpy(want)), (R, name, "noise")
    assert seen == {0, 1}


def test_sample_rays_refuses_a_grid_it_cannot_walk():
    from lidar4d_amd import _lib, ops
    ro, rd = (t.to(DEV) for t in _flag_rays(3))
    lin = torch.linspace(0.0, 1.0, 8, device=DEV)
    bits = torch.zeros(4, dtype=torch.int32, device=DEV)
    z, flags = torch.full((3, 8), 7.0, device=DEV), torch.full((3, 2), 9, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fn, stream = _lib.lib().l4d_sample_rays, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for occ_res, slab, out, text in ((0, 4, p(flags), "occ_res"), (4, 0, p(flags), "slab"), (4, -3, p(flags), "slab"), (4, 4, None, "slab_flags")):
        assert fn(p(ro), p(rd), p(lin), None, 3, 8, NEAR, FAR, 1.0, p(z), None, p(bits), occ_res, slab, out, stream) == 1
        assert text in _lib.lib().l4d_last_error().decode()
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((flags == 9).all())  # refused before anything was launched
    # occ null: the other three are ignored
    assert fn(p(ro), p(rd), p(lin), None, 3, 8, NEAR, FAR, 1.0, p(z), None, None, 0, 0, None, stream) == 0
    assert torch.equal(z, ops.sample_rays(ro, rd, lin, None, NEAR, FAR, 1.0, want_xyz=False)[0])
    for bad in (None, 0, 2.0, True):
        with pytest.raises(ValueError, match="slab"):
            ops.sample_rays(ro, rd, lin, None, NEAR, FAR, 1.0, occ=(bits, 4), slab=bad)
    with pytest.raises(ValueError, match="fewer than"):
        ops.sample_rays(ro, rd, lin, None, NEAR, FAR, 1.0, occ=(bits, 6), slab=4)
    with pytest.raises(TypeError):
        ops.sample_rays(ro, rd, lin, None, NEAR, FAR, 1.0, occ=(bits.long(), 4), slab=4)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(density_scale, g):
    from lidar4d_amd import LiDAR4D
    model = build_scene(LiDAR4D, density_scale, g).to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def _rays(N=N_RAYS):
    ro, rd = make_rays(N, RAY_SEED)
    return ro.to(DEV), rd.to(DEV), torch.tensor([[TIME]], device=DEV)


def _grid(mask, **kw):
    from lidar4d_amd.occupancy import OccupancyGrid
    return OccupancyGrid.from_mask(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV), BOUND, **kw)


@functools.lru_cache(maxsize=None)
def _no_grid(eps):
    """The march without a grid on the mixed scene, computed once and shared (not written to)."""
    ro, rd, t = _rays()
    with torch.no_grad():
        return _model(MIXED_SCALE, G).render(ro, rd, t, num_steps=T_STEPS, early_stop=eps, slab=SLAB)


@functools.lru_cache(maxsize=None)
def _dense():
    """sigma [N, T] fp32 and h [N * T, 16] fp16 of every sample of the rays: ONE full-length slab of the march's own stages (the
    calls of ``early_stop.run`` on all rows at once), and z_vals.  Computed once and shared (not written to)."""
    from lidar4d_amd import occupancy, ops
    model = _model(MIXED_SCALE, G)
    ro, rd, t = _rays()
    t_dev = t.reshape(1).float()
    with torch.no_grad():
        z, xt = ops.sample_rays_xt(ro.view(-1, 3), rd.view(-1, 3), model._lin(T_STEPS, ro.device), None, t_dev, float(np.float32(NEAR)),
                                   float(np.float32(FAR)), BOUND)
        sigma, h = occupancy.field_sigma(model, xt, t_dev, ops.time_setup(t_dev, model.num_frames), rows_like_points=N_RAYS * T_STEPS)
    return sigma.view(N_RAYS, T_STEPS), h, z


def _sample_dist():
    return float((np.float32(FAR) - np.float32(NEAR)) / np.float32(T_STEPS))


# ---- 2. all set, all clear -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-3])
def test_all_set_grid_is_the_march_without_a_grid(eps):
    model, want = _model(MIXED_SCALE, G), _no_grid(eps)
    ro, rd, t = _rays()
    with torch.no_grad():
        out = model.render(ro, rd, t, num_steps=T_STEPS, early_stop=eps, slab=SLAB, occupancy=_grid(np.ones((5, 5, 5), bool)))
    assert set(out) == set(want)
    for k in KEYS:
        assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape and torch.equal(out[k], want[k]), k
    assert torch.equal(_mask_list(out), _mask_list(want))
    assert int(out["evaluated_samples"]) == (N_RAYS * T_STEPS if eps == 0 else int(out["retired_at"].sum()))


@pytest.mark.parametrize("eps", [0.0, 1e-3])
def test_all_clear_grid_renders_nothing(eps):
    model = _model(MIXED_SCALE, G)
    ro, rd, t = _rays()
    with torch.no_grad():
        out = model.render(ro, rd, t, num_steps=T_STEPS, early_stop=eps, slab=SLAB, occupancy=_grid(np.zeros((5, 5, 5), bool)))
    for k in ("depth_lidar", "weights", "weights_sum_lidar", "image_lidar"):
        assert bool((out[k] == 0).all()), k
    assert int(out["mask_count"]) == 0 and int(out["evaluated_samples"]) == 0 and bool((out["retired_at"] == T_STEPS).all())
    assert torch.equal(out["z_vals"], _no_grid(eps)["z_vals"])
    assert float(_no_grid(eps)["depth_lidar"].abs().max()) > 0  # (what ignoring the keyword would have returned)


# ---- 3. shell and blocks against the float64 march ----------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("name", sorted(oref.MARCH_MASKS))
def test_march_against_the_float64_reference(name, eps):
    """The reference marches in float64 over the dense sigma of one full-length slab and says which samples are evaluated and where
    each ray retires; rays whose transmittance comes within 1e-3 of eps at a slab end are exempt from that (at most 5 % of them: the
    early-stop tests' own band and share) and take the device's point.  Everything else is then exact: the outputs are the plain
    stages' (``composite_fwd``, the attribute stage) on the reference's masked sigma, bit for bit."""
    from lidar4d_amd import ops
    from lidar4d_amd.fused import attribute_stage
    model = _model(MIXED_SCALE, G)
    mask = oref.MARCH_MASKS[name]()
    ro, rd, t = _rays()
    sigma, h, z = _dense()
    with torch.no_grad():
        out = model.render(ro, rd, t, num_steps=T_STEPS, early_stop=eps, slab=SLAB, occupancy=_grid(mask))
        again = model.render(ro, rd, t, num_steps=T_STEPS, early_stop=eps, slab=SLAB, occupancy=_grid(mask, time=TIME))
    assert torch.equal(out["z_vals"], z)
    lin = model._lin(T_STEPS, ro.device).cpu().numpy()
    z_ref, flags = oref.slab_flags(mask, ro.view(-1, 3).cpu().numpy(), rd.view(-1, 3).cpu().numpy(), lin, NEAR, FAR, BOUND, SLAB)
    assert np.array_equal(z_ref, z.cpu().numpy())
    dist = _sample_dist()
    sg = sigma.cpu().numpy()
    masked, at, near, rows = oref.march(sg, z_ref, flags, SLAB, eps, dist, MIXED_SCALE, False)
    got_at = out["retired_at"].cpu().numpy()
    print(name, eps, "retired_at:", dict(zip(*[a.tolist() for a in np.unique(got_at, return_counts=True)])), "exempt:", int(near.sum()),
          "evaluated:", int(out["evaluated_samples"]), "reference:", rows, "no grid:", int(_no_grid(eps)["evaluated_samples"]))
    assert near.sum() <= 0.05 * N_RAYS
    assert np.array_equal(got_at[~near], at[~near]), (got_at, at)
    if near.any():  # the exempt rays at the device's retirement point
        at = np.where(near, got_at, at)
        evaluated = ~oref.skipped_samples(flags, SLAB, T_STEPS) & (np.arange(T_STEPS)[None, :] < at[:, None])
        masked, rows = np.where(evaluated, sg, np.float32(0)), int(evaluated.sum())
    assert int(out["evaluated_samples"]) == rows < int(_no_grid(eps)["evaluated_samples"])
    assert 0 < rows and (eps == 0) == bool((got_at == T_STEPS).all())
    with torch.no_grad():
        weights, wsum, depth, _, idx, count = ops.composite_fwd(torch.from_numpy(masked).to(DEV), z, dist, MIXED_SCALE, False,
                                                                want_mask=False, want_idx=True)
        image = attribute_stage(model, rd.view(-1, 3), h, weights, idx, count, T_STEPS, False)[0]
    assert torch.equal(out["weights"], weights) and torch.equal(out["weights_sum_lidar"], wsum)
    assert torch.equal(out["depth_lidar"].view(-1), depth.view(-1)) and torch.equal(out["image_lidar"].view(-1, 2), image.view(-1, 2))
    assert torch.equal(out["mask_count"], count) and torch.equal(_mask_list(out), torch.sort(idx[:int(count)]).values)
    assert int(count) > 100  # (surfaces are hit)
    # weights are zero on every skipped or culled sample, and the float64 composite of the masked sigma agrees to float32 rounding:
    # a factor (1 - alpha) + 1e-15 with alpha = 1 - exp(.) is formed to about 2^-24 ABSOLUTE and every factor is at most 1, so the
    # transmittance in front of sample s is off by at most s * 2^-24 and some, and a weight alpha * T by at most 2 (T + 1) 2^-24
    w64 = oref.composite(masked, z_ref, dist, MIXED_SCALE, False)[0]
    assert bool((out["weights"].cpu().numpy()[masked == 0] == 0).all())
    err = float(np.abs(out["weights"].cpu().numpy() - w64).max())
    print("weights against the float64 composite:", err)
    assert err <= 2 * (T_STEPS + 1) * 2.0 ** -24
    for k in KEYS:  # the same bits twice (a grid that names the call's time is accepted)
        assert torch.equal(out[k], again[k]), k


# ---- 4. build ----------------------------------------------------------------------------------------------------------------------
def _dilated(m, d):
    if d == 0:
        return m
    R = m.shape[0]
    pad = np.zeros((R + 2 * d,) * 3, bool)
    pad[d:R + d, d:R + d, d:R + d] = m
    out = np.zeros_like(m)
    for dz in range(2 * d + 1):
        for dy in range(2 * d + 1):
            for dx in range(2 * d + 1):
                out |= pad[dz:dz + R, dy:dy + R, dx:dx + R]
    return out


def test_build_against_density_at_the_probes():
    """The restatement: ``model.density()`` -- the operator-level path, other kernels than the march's -- at the same probes, the largest
    value per cell, the same product and threshold.  min_depth is four times the median probe value (on the CPU oracle 89 % of the
    cells are then set, tests/test_occupancy_cpu.py's scene).  Cells whose largest probe lies within BAND of min_depth are left
    out, at most 1 % of the cells: BAND is the sigma parity test's tolerance (tests/test_gpu_model.py: sigma = exp(h0) moves by one
    fp16 unit of h0 where the accumulation order flips its last bit, 2^-8 for |h0| < 8) at this threshold's h0 = ln(4 median)
    = 17.5, in [16, 32), where an fp16 unit is 2^-6: exp(2^-6) - 1 < 2^-5.9.  (On the oracle 0.5 % of the cells lie within 2^-6.)"""
    from lidar4d_amd.occupancy import OccupancyGrid
    model = _model(MIXED_SCALE, G)
    R, probes, T = 12, 2, 96
    t = torch.tensor([[TIME]], device=DEV)
    cells = torch.arange(R ** 3, device=DEV)
    c = torch.stack([cells % R, (cells // R) % R, cells // (R * R)], 1).float()
    vals = []
    with torch.no_grad():
        for az in range(probes):
            for ay in range(probes):
                for ax in range(probes):
                    u = (c + torch.tensor([(k + 0.5) / probes for k in (ax, ay, az)], device=DEV)) / float(R)
                    rows = OccupancyGrid.probe_rows(cells, R, probes, (ax, ay, az), TIME)
                    assert torch.equal(rows[:, :3], u) and bool((rows[:, 3] == TIME).all())
                    vals.append(model.density(u * (2 * BOUND) - BOUND, t)["sigma"].float())
    dist = float((np.float32(FAR) - np.float32(NEAR)) / np.float32(T))
    depth = torch.stack(vals).double().cpu().numpy() * MIXED_SCALE * dist          # [probes^3, R^3] per-sample optical depths
    min_depth = 4.0 * float(np.median(depth))
    h0 = np.log(min_depth / (MIXED_SCALE * dist))
    assert 16 <= h0 < 32
    BAND = float(np.exp(2.0 ** -6) - 1.0)
    top = depth.max(0)
    want = (top >= min_depth).reshape(R, R, R)
    border = (np.abs(top / min_depth - 1.0) <= BAND).reshape(R, R, R)
    with torch.no_grad():
        grid = OccupancyGrid.build(model, t, num_steps=T, resolution=R, probes=probes, min_depth=min_depth, dilate=0, max_rows=1000)
        wide = OccupancyGrid.build(model, TIME, num_steps=T, resolution=R, probes=probes, min_depth=min_depth, dilate=1)
    got = grid.mask().cpu().numpy()
    print("set", got.mean(), "reference", want.mean(), "border cells", border.mean(), "differ", (got != want).mean())
    assert (grid.R, grid.bound, grid.time, grid.num_steps, grid.min_depth) == (R, BOUND, TIME, T, min_depth)
    assert grid.bits.is_cuda and grid.bits.dtype == torch.int32 and grid.bits.numel() == R ** 3 // 32
    assert border.mean() <= 0.01 and 0.2 < want.mean() < 0.98
    assert np.array_equal(got[~border], want[~border])
    assert np.array_equal(wide.mask().cpu().numpy(), _dilated(got, 1))             # (batches of 1000 rows or one: the same bits)
    with torch.no_grad():
        coarse = OccupancyGrid.build(model, TIME, num_steps=T, resolution=R, probes=probes, min_depth=0.0, dilate=0)
        none = OccupancyGrid.build(model, TIME, num_steps=T, resolution=R, probes=1, min_depth=float("inf"), dilate=3)
    assert bool(coarse.mask().all()) and not bool(none.mask().any())


# ---- 5. the audit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(oref.MARCH_MASKS))
def test_audit_bounds_the_render_that_skips(name):
    model = _model(MIXED_SCALE, G)
    mask = oref.MARCH_MASKS[name]()
    grid = _grid(mask)
    ro, rd, t = _rays()
    with torch.no_grad():
        plain = model.render(ro, rd, t, num_steps=T_STEPS, perturb=False)
        skipping = model.render(ro, rd, t, num_steps=T_STEPS, early_stop=0.0, slab=SLAB, occupancy=grid)
        a = grid.audit(model, ro, rd, t, T_STEPS, SLAB)
    # the audit's full render is the plain render
    assert torch.equal(a["weights"], plain["weights"]) and torch.equal(a["z_vals"], plain["z_vals"])
    assert torch.equal(a["weights_sum"], plain["weights_sum_lidar"]) and torch.equal(a["depth"].view(-1), plain["depth_lidar"].view(-1))
    # its flags, D and lost weight are the reference's on the dense sigma
    sigma, _, z = _dense()
    lin = model._lin(T_STEPS, ro.device).cpu().numpy()
    _, flags = oref.slab_flags(mask, ro.view(-1, 3).cpu().numpy(), rd.view(-1, 3).cpu().numpy(), lin, NEAR, FAR, BOUND, SLAB)
    assert np.array_equal(a["flags"].cpu().numpy(), flags)
    skipped = oref.skipped_samples(flags, SLAB, T_STEPS)
    tau = oref.optical_depth(sigma.cpu().numpy(), z.cpu().numpy(), _sample_dist(), MIXED_SCALE, False)
    D = np.where(skipped, tau, 0.0).sum(1)
    lost = np.where(skipped, plain["weights"].double().cpu().numpy(), 0.0).sum(1)
    assert a["D"].dtype == torch.float64 and np.allclose(a["D"].cpu().numpy(), D, rtol=1e-12, atol=0)
    assert np.allclose(a["skipped_weight"].cpu().numpy(), lost, rtol=1e-12, atol=0)
    print(name, "D: min %.3g median %.3g max %.3g" % (D.min(), np.median(D), D.max()), "rays with D <= D_MAX:", int((D <= oref.D_MAX).sum()))
    assert (D > 0).any()
    np_ = lambda o: {"weights": o["weights"].cpu().numpy(), "weights_sum": o["weights_sum_lidar"].cpu().numpy(),
                     "depth": o["depth_lidar"].reshape(-1).cpu().numpy()}
    oref.check_audit(np_(plain), np_(skipping), D, lost, skipped, float(model.far_lidar), slack=er.REL, what=name)
    # samples with nothing skipped in front of them: the full render's bits
    front = np.cumsum(skipped, axis=1) == 0
    print("samples with nothing skipped in front:", int(front.sum()), "rays with D <= 1:", int((D <= 1.0).sum()))
    assert front.any()
    front = torch.from_numpy(front).to(DEV)
    assert torch.equal(skipping["weights"][front], plain["weights"][front])


# ---- 6. staged renders and the callers ------------------------------------------------------------------------------------------
def test_staged_render_is_the_chunks_one_after_the_other():
    model = _model(MIXED_SCALE, G)
    grid = _grid(oref.MARCH_MASKS["shell"](), time=TIME)
    ro, rd, t = _rays()
    kw = dict(num_steps=T_STEPS, early_stop=1e-3, slab=SLAB, occupancy=grid)
    with torch.no_grad():
        staged = model.render(ro, rd, t, staged=True, max_ray_batch=16, **kw)
        chunks = [model.render(ro[:, a:a + 16], rd[:, a:a + 16], t, **kw) for a in range(0, N_RAYS, 16)]
    assert set(staged) == {"depth_lidar", "image_lidar", "evaluated_samples", "retired_at"}
    assert staged["depth_lidar"].shape == (1, N_RAYS) and staged["image_lidar"].shape == (1, N_RAYS, 2)
    for k in ("depth_lidar", "image_lidar", "retired_at"):
        assert torch.equal(staged[k], torch.cat([c[k] if k == "image_lidar" else c[k].reshape(1, -1) for c in chunks], 1)), k
    assert int(staged["evaluated_samples"]) == sum(int(c["evaluated_samples"]) for c in chunks) < N_RAYS * T_STEPS
    with torch.no_grad(), pytest.raises(ValueError, match="occupancy needs early_stop"):
        model.render(ro, rd, t, staged=True, max_ray_batch=16, num_steps=T_STEPS, occupancy=grid)


def test_simulator_and_evaluate_build_the_grid_per_frame(monkeypatch):
    """A field of uniform density (the filled model at density_scale 40: per-sample optical depth 0.2 and more everywhere) gives a grid
    that is all set: with the keyword the callers return what they return without it."""
    from lidar4d_amd import LiDAR4D, occupancy
    from lidar4d_amd.data import KITTI360_FOV, KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.simulator import Simulator
    from lidar4d_amd.trainer import Trainer
    from oracle.detparams import fill_model
    torch.manual_seed(0)
    H, W, T = 16, 64, 96
    data = SyntheticKitti360(DEV, H=H, W=W, num_frames=5, num_rays=256)
    cfg = dict(SMALL_MODEL, num_frames=5, near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE, density_scale=OPAQUE_SCALE)
    model = fill_model(LiDAR4D(**cfg), seed=7).to(DEV).eval()
    built = []
    inner = occupancy.OccupancyGrid.build.__func__

    def recording_build(cls, *a, **kw):
        grid = inner(cls, *a, **kw)
        built.append(grid)
        return grid

    monkeypatch.setattr(occupancy.OccupancyGrid, "build", classmethod(recording_build))
    tr = Trainer(model, data, num_steps=T)
    opts = dict(early_stop=5e-5, slab=16)
    plain = tr.evaluate(frames=[1, 3], refine=False, max_ray_batch=300, **opts)
    skip = tr.evaluate(frames=[1, 3], refine=False, max_ray_batch=300, occupancy={"resolution": 8}, **opts)
    assert len(built) == 2 and [g.time for g in built] == [float(data.frame(k)["time"].reshape(-1)[0]) for k in (1, 3)]
    assert all(bool(g.mask().all()) and g.R == 8 and g.num_steps == T and g.min_depth == 1e-3 for g in built)
    assert skip["loss"] == plain["loss"]
    for k in ("raydrop", "intensity", "depth"):
        np.testing.assert_array_equal(np.asarray(skip[k]), np.asarray(plain[k]))
    # (the points meter: fp32 means of chamfer distances whose order the library does not promise, as in tests/test_gpu_meters.py)
    np.testing.assert_allclose(skip["points"], plain["points"], rtol=1e-6, atol=0, equal_nan=True)
    a = tr.collect_refine_data(frames=[2], max_ray_batch=300, **opts)
    b = tr.collect_refine_data(frames=[2], max_ray_batch=300, occupancy={"resolution": 8, "probes": 1}, **opts)
    assert len(built) == 3 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    del built[:]
    fr = data.frame(2)
    seen = {}

    def capture(key):
        def to_points(depth_m, intensity, fov):
            seen[key] = (depth_m.clone(), intensity.clone())
            return depth_m
        return to_points

    opt = types.SimpleNamespace(scale=KITTI360_SCALE, fov_lidar=KITTI360_FOV, num_steps=T, max_ray_batch=300)
    for key, kw in (("plain", {}), ("skip", {"occupancy": {"resolution": 8}})):
        sim = Simulator("occ", opt, model, device=torch.device(DEV), mute=True, workspace=None, use_refine=False, H_lidar=H, W_lidar=W,
                        to_points=capture(key), **opts, **kw)
        sim.render(fr["rays_o_lidar"], fr["rays_d_lidar"], fr["time"], save_pc=False, save_img=False, save_video=False)
    assert len(built) == 1 and bool(built[0].mask().all())
    assert torch.equal(seen["skip"][0], seen["plain"][0]) and torch.equal(seen["skip"][1], seen["plain"][1])
