"""CPU side of empty-space skipping (``render(..., early_stop=eps, slab=S, occupancy=grid)``, lidar4d_amd/occupancy.py): the bit
packing against the numpy restatement (tests/occupancy_ref.py), what the option refuses before anything touches a device, the ABI
of the entry point that carries the flags, the keyword in the callers, and the restatement itself -- its flags and march on hand-made
cases, the audit's inequalities on synthetic float64 sigma.  No GPU."""
import inspect
import types

import numpy as np
import pytest
import torch

import occupancy_ref as oref
import test_abi_cpu as abi
from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

TIME = 0.5


# ---- packing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 32, 33])
def test_from_mask_packs_the_reference_bits(R):
    from lidar4d_amd.occupancy import OccupancyGrid
    rng = np.random.default_rng(R)
    masks = {"random": rng.random((R, R, R)) < 0.5, "set": np.ones((R, R, R), bool), "clear": np.zeros((R, R, R), bool),
             "corner": np.zeros((R, R, R), bool)}
    masks["corner"][R - 1, R - 1, R - 1] = True
    for name, m in masks.items():
        grid = OccupancyGrid.from_mask(torch.from_numpy(m), bound=1)
        want = oref.pack(m)
        assert grid.bits.dtype == torch.int32 and grid.bits.shape == ((R ** 3 + 31) // 32,), name
        assert np.array_equal(grid.bits.numpy(), want), name
        assert (grid.R, grid.bound, grid.time, grid.num_steps, grid.min_depth) == (R, 1, None, None, None)
        assert np.array_equal(grid.mask().numpy(), m), name
    # the layout: cell (cx, cy, cz) = mask[cz, cy, cx] is bit i & 31 of word i >> 5, i = (cz R + cy) R + cx
    if R >= 5:
        one = np.zeros((R, R, R), bool)
        one[3, 1, 2] = True
        i = (3 * R + 1) * R + 2
        bits = OccupancyGrid.from_mask(torch.from_numpy(one), bound=1).bits.numpy().view(np.uint32)
        assert bits[i >> 5] == np.uint32(1) << np.uint32(i & 31) and np.count_nonzero(bits) == 1
    for bad in (torch.ones(2, 2, 3, dtype=torch.bool), torch.ones(2, 2, 2), torch.ones(0, 0, 0, dtype=torch.bool), torch.ones(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="bool \\[R, R, R\\]"):
            OccupancyGrid.from_mask(bad, bound=1)


# ---- refusals that need no device ----------------------------------------------------------------------------------------------
def _grid(R=4, **kw):
    from lidar4d_amd.occupancy import OccupancyGrid
    grid = OccupancyGrid.from_mask(torch.ones(R, R, R, dtype=torch.bool), bound=kw.pop("bound", 1), time=kw.pop("time", None))
    grid.num_steps = kw.pop("num_steps", None)
    return grid


def _cpu_call(model, **kw):
    ro, rd = make_rays(5, 3)
    return model.render(ro, rd, torch.tensor([[TIME]]), num_steps=32, **kw)


def test_option_checks_without_a_device():
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.occupancy import OccupancyGrid
    model = LiDAR4D(**SMALL_MODEL)
    with torch.no_grad():
        for kw in ({}, {"staged": True, "max_ray_batch": 2}, {"cull": 1e-4}):
            with pytest.raises(ValueError, match="occupancy needs early_stop"):
                _cpu_call(model, occupancy=_grid(), **kw)
        with pytest.raises(ValueError, match="the grid's bound"):
            _cpu_call(model, early_stop=1e-4, occupancy=_grid(bound=2))
        with pytest.raises(ValueError, match="built for time"):
            _cpu_call(model, early_stop=1e-4, occupancy=_grid(time=0.25))
        with pytest.raises(ValueError, match="built for num_steps=64"):
            _cpu_call(model, early_stop=1e-4, occupancy=_grid(num_steps=64))
        with pytest.raises(ValueError, match="must be None or an OccupancyGrid"):
            _cpu_call(model, early_stop=1e-4, occupancy={"resolution": 4})
        # the pinned refusals of early_stop come first and stay
        with pytest.raises(ValueError, match="perturb=True"):
            _cpu_call(model, early_stop=1e-4, perturb=True, occupancy=_grid())
        narrow = LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=4, n_levels_plane=4))
        assert narrow.fused is False
        with pytest.raises(ValueError, match="needs the fused pipeline"):
            _cpu_call(narrow, early_stop=1e-4, occupancy=_grid())
        with pytest.raises(ValueError, match="occupancy needs early_stop"):
            _cpu_call(narrow, occupancy=_grid())
        with pytest.raises(ValueError, match="occupancy needs the fused pipeline"):
            OccupancyGrid.build(narrow, TIME, num_steps=32, resolution=4)
        with pytest.raises(ValueError, match="occupancy needs the fused pipeline"):
            _grid().audit(narrow, *make_rays(5, 3), TIME, 32, 8)
        with pytest.raises(ValueError, match="at least 1"):
            OccupancyGrid.build(model, TIME, num_steps=32, resolution=0)
        # a matching grid: nothing left to refuse, the march starts -- and has no CPU fallback
        with pytest.raises(Exception, match="no CPU fallback"):
            _cpu_call(model, early_stop=0.0, slab=8, occupancy=_grid(time=TIME, num_steps=32))
        with pytest.raises(Exception, match="no CPU fallback"):
            OccupancyGrid.build(model, TIME, num_steps=32, resolution=4)
    assert torch.is_grad_enabled()
    with pytest.raises(ValueError, match="requires grad"):
        _cpu_call(model, early_stop=1e-4, occupancy=_grid())
    with pytest.raises(ValueError, match="requires grad"):
        OccupancyGrid.build(model, TIME, num_steps=32, resolution=4)


def test_sample_rays_checks_its_grid_arguments():
    from lidar4d_amd import _lib, ops
    assert list(inspect.signature(ops.sample_rays).parameters)[-2:] == ["occ", "slab"]
    ro, rd = (t.view(-1, 3) for t in make_rays(5, 3))
    lin = torch.linspace(0, 1, 8)
    bits = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.sample_rays(ro, rd, lin, None, 0.1, 0.8, 1, occ=(bits, 4), slab=4)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_six_carries_the_flags_on_sample_rays():
    from lidar4d_amd import _lib
    assert _lib.ABI_VERSION == 6
    sig = _lib.SIGNATURES["l4d_sample_rays"]
    assert len(sig) == 16 and sig[-5:] == [_lib.P, _lib.I32, _lib.I32, _lib.P, _lib.P]
    assert "#define L4D_ABI_VERSION 6" in open(abi.os.path.join(abi.ROOT, "include", "lidar4d_hip.h")).read()
    assert len(_lib.BINDINGS) == 9  # no tenth library
    abi.test_ctypes_signatures_match_header_prototypes(abi.ROW["hip"])


# ---- the callers ---------------------------------------------------------------------------------------------------------------
def test_callers_build_one_grid_per_frame_and_hand_it_on(monkeypatch):
    from lidar4d_amd import occupancy
    from lidar4d_amd.simulator import Simulator
    from lidar4d_amd.trainer import Trainer
    for fn in (Trainer.test_step, Trainer.evaluate, Trainer.collect_refine_data, Simulator.__init__):
        assert inspect.signature(fn).parameters["occupancy"].default is None, fn
    built, seen = [], []

    def fake_build(model, time, num_steps=768, **kw):
        built.append((float(time.reshape(-1)[0]), num_steps, kw))
        return ("grid", len(built))

    monkeypatch.setattr(occupancy.OccupancyGrid, "build", staticmethod(fake_build))

    class Model:
        unet = staticmethod(lambda x: x[:, :1].squeeze(0))

        def render(self, rays_o, rays_d, time, **kw):
            seen.append(kw)
            n = rays_o.shape[1]
            return {"depth_lidar": torch.zeros(1, n), "image_lidar": torch.zeros(1, n, 2)}

    tr = Trainer.__new__(Trainer)
    tr.model, tr.num_steps = Model(), 32
    data = {"rays_o_lidar": torch.zeros(1, 8, 3), "rays_d_lidar": torch.zeros(1, 8, 3), "time": torch.full((1, 1), 0.25), "H_lidar": 2, "W_lidar": 4}
    tr.test_step(data, refine=False)
    tr.test_step(data, refine=False, early_stop=0.0, slab=16, occupancy={"resolution": 8, "dilate": 0})
    assert "occupancy" not in seen[0] and built == [(0.25, 32, {"resolution": 8, "dilate": 0})]
    assert seen[1]["occupancy"] == ("grid", 1) and seen[1]["early_stop"] == 0.0 and seen[1]["slab"] == 16
    del seen[:], built[:]
    times = torch.tensor([[0.25], [0.75]])
    for kw, n_grids in (({}, 0), ({"early_stop": 1e-4, "slab": 48, "occupancy": {"resolution": 16}}, 2)):
        sim = Simulator("t", types.SimpleNamespace(scale=1.0, fov_lidar=(2.0, 26.9), num_steps=32), Model(), device=torch.device("cpu"),
                        mute=True, workspace=None, use_refine=False, H_lidar=2, W_lidar=4, to_points=lambda d, i, fov: d, **kw)
        sim.render(torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), times, save_pc=False, save_img=False, save_video=False)
        assert len(built) == n_grids
    assert [b[:2] for b in built] == [(0.25, 32), (0.75, 32)]  # one per frame, at that frame's time
    assert [kw.get("occupancy") for kw in seen] == [None, None, ("grid", 1), ("grid", 2)]
    with pytest.raises(ValueError, match="must be None or a dict"):
        tr.test_step(data, refine=False, early_stop=0.0, occupancy=7)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_reference_flags_on_hand_made_rays():
    R, T = 4, 8
    lin = np.linspace(0.0, 1.0, T, dtype=np.float32)
    o = np.array([[-0.9, 0.1, 0.1], [3.0, 3.0, 3.0]], np.float32)   # along +x through the row y = z = 2; outside the box
    d = np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 1.0]], np.float32)
    mask = np.zeros((R, R, R), bool)
    mask[2, 2, 3] = True                                               # the cell x in [0.5, 1]
    z, flags = oref.slab_flags(mask, o, d, lin, 0.0, 1.75, 1.0, 2)
    # ray 0: x = -0.9 + z, z = 0, .25, ... 1.75 -> cells 0 0 0 1 2 2 3 3; ray 1: clipped to the corner (1, 1, 1) -> cell (3, 3, 3)
    assert z.dtype == np.float32 and flags.tolist() == [[0, 0, 0, 1], [0, 0, 0, 0]]
    corner = np.zeros((R, R, R), bool)
    corner[3, 3, 3] = True
    assert oref.slab_flags(corner, o, d, lin, 0.0, 1.75, 1.0, 3)[1].tolist() == [[0, 0, 0], [1, 1, 1]]
    assert oref.slab_flags(corner, o, d, lin, 0.0, 1.75, 1.0, 1000)[1].tolist() == [[0], [1]]
    _, cell = oref.sample_cells(o, d, lin, 0.0, 1.75, 1.0, 1)
    assert (cell == 0).all()


def test_reference_march_skips_and_retires():
    T, S = 12, 4
    z = np.tile(np.linspace(0.1, 1.2, T), (4, 1))
    sigma = np.zeros((4, T))
    sigma[:, 1], sigma[:, 5], sigma[:, 9] = 3.0, 1e4, 1e4   # thin in slab 0, opaque in slabs 1 and 2
    flags = np.array([[1, 1, 1], [1, 0, 1], [0, 0, 0], [1, 1, 0]], np.uint8)
    masked, at, near, n = oref.march(sigma, z, flags, S, 1e-3, 0.1, 1.0, False)
    assert at.tolist() == [8, 12, 12, 8] and not near.any() and n == 8 + 8 + 0 + 8
    assert (masked[0, :8] == sigma[0, :8]).all() and (masked[0, 8:] == 0).all()
    assert (masked[1, 4:8] == 0).all() and masked[1, 9] == 1e4 and (masked[2] == 0).all()
    masked, at, _, n = oref.march(sigma, z, flags, S, 0.0, 0.1, 1.0, False)
    assert at.tolist() == [12] * 4 and n == 12 + 8 + 0 + 8
    assert np.array_equal(masked, np.where(oref.skipped_samples(flags, S, T), 0.0, sigma))
    # a ray exactly at the threshold's band is reported
    tau = 3.0 * (z[0, 2] - z[0, 1])
    _, _, near, _ = oref.march(sigma[:1], z[:1], flags[:1], S, float(np.exp(-tau)) * (1 + 5e-4), 0.1, 1.0, False)
    assert near.tolist() == [True]


def test_march_masks_skip_and_evaluate_less_on_the_oracle():
    """The scene and masks tests/test_gpu_occupancy.py marches through, on the CPU oracle's density: each mask skips slabs, no ray is
    near the threshold, and at both eps fewer rows are evaluated than without a grid.  Measured (rows at eps 0 / 1e-3; no grid
    4810 / 2016): shell 2496 / 1856, blocks 1984 / 1228."""
    from oracle import fields_ref, tcnn_ref
    from test_early_stop_cpu import G, MIXED_SCALE, RAY_SEED, build_scene
    N, T, S = 37, 130, 32
    near, far = np.float32(SMALL_MODEL["near_lidar"]), np.float32(SMALL_MODEL["far_lidar"])
    ro, rd = (t.view(-1, 3).numpy() for t in make_rays(N, RAY_SEED))
    lin = torch.linspace(0.0, 1.0, T).numpy()
    z, _ = oref.sample_cells(ro, rd, lin, near, far, 1.0, 1)
    x = np.clip(ro[:, None, :] + rd[:, None, :] * z[:, :, None], -1.0, 1.0).reshape(-1, 3)
    prev = tcnn_ref.get_precision()
    tcnn_ref.set_precision("tcnn")
    try:
        with torch.no_grad():
            sigma = build_scene(fields_ref.LiDAR4D, MIXED_SCALE, G).density(torch.from_numpy(x), torch.tensor([[TIME]]))["sigma"]
    finally:
        tcnn_ref.set_precision(prev)
    sigma = sigma.float().numpy().reshape(N, T)
    dist = float((far - near) / np.float32(T))
    for eps in (0.0, 1e-3):
        _, _, near_eps, plain = oref.march(sigma, z, np.ones((N, 5), np.uint8), S, eps, dist, MIXED_SCALE, False)
        assert not near_eps.any() and (plain == N * T) == (eps == 0.0)
        for name, make in oref.MARCH_MASKS.items():
            _, flags = oref.slab_flags(make(), ro, rd, lin, near, far, 1.0, S)
            masked, at, near_eps, rows = oref.march(sigma, z, flags, S, eps, dist, MIXED_SCALE, False)
            print(name, eps, "rows", rows, "of", plain, "flags", int(flags.sum()), "of", flags.size)
            assert 0 < flags.sum() < flags.size and not near_eps.any()
            assert 0 < rows < plain - 2 * S, (name, eps, rows, plain)
            assert (oref.composite(masked, z, dist, MIXED_SCALE, False)[0] > 1e-4).sum() > 100  # (and surfaces are still hit)
            if eps > 0:
                assert (at < T).any() and (at == T).any()


@pytest.mark.parametrize("active", [False, True], ids=["passive", "active"])
@pytest.mark.parametrize("kind", ["random", "zero_on_skipped", "dense_skipped"])
def test_audit_inequalities_on_synthetic_sigma(kind, active):
    """The bound that ``OccupancyGrid.audit`` states, on float64 composites of synthetic sigma: the render that skips is the composite
    of sigma zeroed on the skipped slabs.  And ``occupancy.skipped_depth`` is the restatement's D and lost weight."""
    from lidar4d_amd.occupancy import skipped_depth
    rng = np.random.default_rng(3)
    N, T, S, far = 40, 130, 32, 0.85
    z = np.sort(rng.uniform(0.01, far, (N, T)), axis=1)
    sigma = rng.uniform(0.0, 4.0, (N, T)) * rng.choice([0.01, 1.0, 30.0], (N, 1))
    flags = (rng.random((N, -(-T // S))) < 0.5).astype(np.uint8)
    flags[0], flags[1] = 1, 0
    skipped = oref.skipped_samples(flags, S, T)
    if kind == "zero_on_skipped":
        sigma[skipped] = 0.0
    if kind == "dense_skipped":
        sigma[skipped] *= 50.0
    dist, scale = 0.0065, 1.3
    w, ws, dep = oref.composite(sigma, z, dist, scale, active)
    w2, ws2, dep2 = oref.composite(np.where(skipped, 0.0, sigma), z, dist, scale, active)
    D = np.where(skipped, oref.optical_depth(sigma, z, dist, scale, active), 0.0).sum(1)
    lost = np.where(skipped, w, 0.0).sum(1)
    oref.check_audit({"weights": w, "weights_sum": ws, "depth": dep}, {"weights": w2, "weights_sum": ws2, "depth": dep2}, D, lost, skipped,
                     far, slack=1e-9, t_abs=0.0, what=kind)
    if kind == "zero_on_skipped":
        assert (D == 0).all() and np.array_equal(w, w2)
    else:
        assert D[1] > 0 and D[0] == 0 and ws2[1] == 0
    # exactly e^{D_s}: the factor is the skipped optical depth in front of the sample
    tau = oref.optical_depth(sigma, z, dist, scale, active)
    D_front = np.cumsum(np.where(skipped, tau, 0.0), axis=1) - np.where(skipped, tau, 0.0)
    ev = ~skipped & (w > 1e-200) & (D_front <= oref.D_MAX)
    assert ev.any() and np.allclose(w2[ev], (w * np.exp(np.minimum(D_front, oref.D_MAX)))[ev], rtol=1e-9, atol=0)
    got_D, got_lost = skipped_depth(torch.from_numpy(sigma), torch.from_numpy(z), torch.from_numpy(w), torch.from_numpy(skipped), dist, scale, active)
    assert np.allclose(got_D.numpy(), D, rtol=1e-12, atol=0) and np.allclose(got_lost.numpy(), lost, rtol=1e-12, atol=0)
