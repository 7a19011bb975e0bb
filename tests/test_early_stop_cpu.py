"""CPU side of early ray termination (``render(..., early_stop=eps, slab=S)``): what the
option cannot do is refused by name before anything touches a device; without the option the render goes through the same function
as before (``RenderFn.apply``); the numpy restatement of the retirement rule (tests/early_stop_ref.py) is pinned; and on the CPU oracle
the scenes the GPU tests use retire rays where they are said to, with the culled weights inside the bound.  No GPU."""
import types

import numpy as np
import pytest
import torch

import early_stop_ref as er
import test_abi_cpu as abi
from oracle import fields_ref
from oracle.detparams import fill_model
from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

# The scenes (tests/test_gpu_early_stop.py renders the same ones): SMALL_MODEL, fill_model(seed=7), make_rays(64, 36), t = 0.5,
# T = 96, S = 16.  MIXED: row 0 of the density network's output matrix (the one that makes sigma) times G, with the density_scale that
# goes with it.  The gain is what gives the field contrast along a ray (log sigma = G * h0 with h0 = -0.25 +- 0.07 on these rays):
# at G = -60 sigma spans e^8 along a ray, rays end at surfaces in different slabs and some meet none.  SMOOTH and STEEP are the
# low-contrast scenes G = -12 and G = -16 at density_scale 0.5, where T falls by a steady factor per slab.
N_RAYS, RAY_SEED, T_STEPS, SLAB, TIME = 64, 36, 96, 16, 0.5
G, MIXED_SCALE, OPAQUE_SCALE = -60.0, 1e-7, 40.0
SMOOTH, STEEP = (0.5, -12.0), (0.5, -16.0)


def scale_density_row(model, g):
    """Row 0 of the density network's [16, hidden] output matrix -- the first ``hidden`` of the last ``16 * hidden`` parameters -- times g."""
    p, hidden = model.sigma_net.params, model.sigma_net.n_neurons
    with torch.no_grad():
        p[p.numel() - 16 * hidden:p.numel() - 15 * hidden] *= g
    return model


def build_scene(cls, density_scale, g=None, **extra):
    model = fill_model(cls(**dict(SMALL_MODEL, density_scale=density_scale, **extra)), seed=7)
    return model if g is None else scale_density_row(model, g)


_ORACLE = {}


def oracle_render(density_scale, g):
    """The oracle's full render of a scene (tcnn rounding), computed once."""
    key = (density_scale, g)
    if key not in _ORACLE:
        from oracle import tcnn_ref
        prev = tcnn_ref.get_precision()
        tcnn_ref.set_precision("tcnn")
        try:
            model = build_scene(fields_ref.LiDAR4D, density_scale, g)
            ro, rd = make_rays(N_RAYS, RAY_SEED)
            with torch.no_grad():
                out = model.render(ro, rd, torch.tensor([[TIME]]), num_steps=T_STEPS, perturb=False)
            _ORACLE[key] = ({k: v.numpy() for k, v in out.items()}, float(model.far_lidar))
        finally:
            tcnn_ref.set_precision(prev)
    return _ORACLE[key]


# Kept under their earlier names, as calls of the checks in tests/test_abi_cpu.py, which run there for every library: a new library
# adds no test of this kind.
def test_march_ctypes_signatures_match_header_prototypes():
    abi.test_ctypes_signatures_match_header_prototypes(abi.ROW["march"])


def test_march_library_exports_no_name_of_another():
    abi.test_no_library_exports_a_name_of_another()


# ---- refusals that need no device --------------------------------------------------------------------------------------------
def _cpu_call(model, **kw):
    ro, rd = make_rays(5, 3)
    return model.render(ro, rd, torch.tensor([[TIME]]), num_steps=32, **kw)


def test_refusals_without_a_device():
    from lidar4d_amd import LiDAR4D
    model = LiDAR4D(**SMALL_MODEL)
    with torch.no_grad():
        for bad in (-1e-6, float("nan"), float("inf"), "1e-4", True):
            with pytest.raises(ValueError, match="early_stop must be"):
                _cpu_call(model, early_stop=bad)
        for bad in (0, -16, 1.5, None):
            with pytest.raises(ValueError, match="slab must be a positive int"):
                _cpu_call(model, early_stop=1e-4, slab=bad)
        with pytest.raises(ValueError, match="perturb=True"):
            _cpu_call(model, early_stop=1e-4, perturb=True)
        with pytest.raises(ValueError, match="perturb=True"):
            _cpu_call(model, early_stop=1e-4, perturb=True, staged=True, max_ray_batch=2)
        narrow = LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=4, n_levels_plane=4))
        assert narrow.fused is False
        with pytest.raises(ValueError, match="needs the fused pipeline"):
            _cpu_call(narrow, early_stop=1e-4)
    assert torch.is_grad_enabled()
    with pytest.raises(ValueError, match="requires grad"):
        _cpu_call(model, early_stop=1e-4)
    for p in model.parameters():
        p.requires_grad_(False)
    # nothing left to refuse: with grad mode on and no parameter requiring grad, the march starts -- and has no CPU fallback
    with pytest.raises(Exception, match="no CPU fallback"):
        _cpu_call(model, early_stop=1e-4)
    with torch.no_grad(), pytest.raises(Exception, match="no CPU fallback"):
        _cpu_call(model, early_stop=0.0, slab=7)


def test_generic_renderer_refuses_early_stop():
    from lidar4d_amd.renderer import LiDAR_Renderer
    ro, rd = make_rays(5, 3)
    with pytest.raises(ValueError, match="needs the fused pipeline"):
        LiDAR_Renderer().run(ro, rd, torch.tensor([[TIME]]), num_steps=8, early_stop=1e-4)


def test_without_the_option_the_launch_path_is_renderfn_apply(monkeypatch):
    """``early_stop=None`` (the default everywhere) goes through ``RenderFn.apply`` as before and never into early_stop.run; with
    the option set it is the other way round."""
    from lidar4d_amd import LiDAR4D, early_stop, fused, lidar4d
    assert lidar4d.RenderFn is fused.RenderFn
    calls = []

    def seven(N, num_steps):
        return (torch.zeros(N), torch.zeros(N, 2), torch.zeros(N), torch.zeros(N, num_steps), torch.zeros(N, num_steps),
                torch.zeros(N * num_steps, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))

    def fake_apply(model, rays_o, rays_d, t_dev, noise, num_steps, train, *params):
        calls.append(("apply", rays_o.shape[0], num_steps, train))
        return seven(rays_o.shape[0], num_steps)

    def fake_run(model, rays_o, rays_d, t_dev, num_steps, eps, S):
        calls.append(("march", rays_o.shape[0], num_steps, eps, S))
        N = rays_o.shape[0]
        return seven(N, num_steps) + (torch.tensor(N * num_steps), torch.full((N,), num_steps, dtype=torch.int32))

    monkeypatch.setattr(lidar4d.RenderFn, "apply", staticmethod(fake_apply))
    monkeypatch.setattr(early_stop, "run", fake_run)
    model = LiDAR4D(**SMALL_MODEL)
    ro, rd = make_rays(5, 3)
    t = torch.tensor([[TIME]])
    with torch.no_grad():
        plain = model.render(ro, rd, t, num_steps=32)
        assert calls == [("apply", 5, 32, False)] and set(plain) == {"depth_lidar", "image_lidar", "weights_sum_lidar", "weights", "z_vals",
                                                                     "mask_idx", "mask_count"}
        model.render(ro, rd, t, num_steps=32, early_stop=None, slab=16)
        model.render(ro, rd, t, num_steps=32, staged=True, max_ray_batch=2)
        assert [c[0] for c in calls] == ["apply"] * 5
        del calls[:]
        out = model.render(ro, rd, t, num_steps=32, early_stop=5e-5)
        assert calls == [("march", 5, 32, 5e-5, 96)]  # (slab's default)
        assert set(out) == set(plain) | {"evaluated_samples", "retired_at"}
        del calls[:]
        model.graph_staged = True  # ignored while early_stop is set
        out = model.render(ro, rd, t, num_steps=32, staged=True, max_ray_batch=2, early_stop=1e-2, slab=8)
        assert calls == [("march", 2, 32, 1e-2, 8), ("march", 2, 32, 1e-2, 8), ("march", 1, 32, 1e-2, 8)]
        assert out["retired_at"].shape == (1, 5) and int(out["evaluated_samples"]) == 5 * 32


def test_trainer_and_simulator_hand_the_keywords_on():
    """Defaults are None (the plain render's call, no extra keyword); a value reaches ``model.render`` with ``slab``."""
    import inspect
    from lidar4d_amd.simulator import Simulator
    from lidar4d_amd.trainer import Trainer
    for fn in (Trainer.test_step, Trainer.evaluate, Trainer.collect_refine_data, Simulator.__init__):
        sig = inspect.signature(fn)
        assert sig.parameters["early_stop"].default is None and sig.parameters["slab"].default == 96, fn
    seen = []

    class Model:
        unet = staticmethod(lambda x: x[:, :1].squeeze(0))

        def render(self, rays_o, rays_d, time, **kw):
            seen.append(kw)
            n = rays_o.shape[1]
            return {"depth_lidar": torch.zeros(1, n), "image_lidar": torch.zeros(1, n, 2)}

    tr = Trainer.__new__(Trainer)
    tr.model, tr.num_steps = Model(), 32
    data = {"rays_o_lidar": torch.zeros(1, 8, 3), "rays_d_lidar": torch.zeros(1, 8, 3), "time": torch.zeros(1, 1), "H_lidar": 2, "W_lidar": 4}
    tr.test_step(data, refine=False)
    tr.test_step(data, refine=False, early_stop=5e-5, slab=64)
    assert "early_stop" not in seen[0] and "slab" not in seen[0]
    assert seen[1]["early_stop"] == 5e-5 and seen[1]["slab"] == 64
    del seen[:]
    for kw, want in (({}, None), ({"early_stop": 1e-4, "slab": 48}, (1e-4, 48))):
        sim = Simulator("t", types.SimpleNamespace(scale=1.0, fov_lidar=(2.0, 26.9), num_steps=32), Model(), device=torch.device("cpu"),
                        mute=True, workspace=None, use_refine=False, H_lidar=2, W_lidar=4, to_points=lambda d, i, fov: d, **kw)
        sim.render(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(1, 1), save_pc=False, save_img=False, save_video=False)
        got = seen.pop()
        assert (got.get("early_stop"), got.get("slab")) == (want if want else (None, None))


# ---- the numpy restatement --------------------------------------------------------------------------------------------------
def test_reference_product_order_and_rule():
    rng = np.random.default_rng(5)
    for n in (1, 16, 63, 64, 65, 96, 128, 192):
        f = rng.uniform(0.8, 1.0, n).astype(np.float32)  # (192 of them stay far above float32's underflow)
        got = er.slab_product(f)
        assert got.dtype == np.float32
        exact = float(np.prod(f.astype(np.float64)))
        assert abs(float(got) - exact) <= 2 * n * 2.0 ** -24 * exact  # the bound's theta
    # lanes past the slab's end hold 1; a factor of exactly 1 changes nothing
    assert er.slab_product(np.ones(100, np.float32)) == np.float32(1.0)
    # the rule: rays that retire after each slab, never, with all-zero sigma (T^ stays exactly 1), with an inf and a NaN
    T, S = 48, 16
    z = np.tile(np.linspace(0.1, 1.0, T, dtype=np.float32), (6, 1))
    sigma = np.zeros((6, T), np.float32)
    sigma[0, 3], sigma[1, 20], sigma[2, 40] = 1e4, 1e4, 1e4   # opaque in slab 0 / 1 / 2
    sigma[3, :] = 1e-3                                          # thin: never
    sigma[4, 5] = np.inf                                        # row 5 stays all-zero
    nan = sigma.copy()
    nan[3, 2] = np.nan
    for active in (False, True):
        f = er.factors(sigma, z, 0.02, 1.0, active)
        assert f.dtype == np.float32 and bool((f[5] == 1).all())
        for eps, want in ((0.0, [48] * 6), (5e-5, [16, 32, 48, 48, 16, 48]), (1.0, [16, 32, 48, 16, 16, 48])):  # (T^ = 1 exactly is not below 1)
            trans, at, lists = er.march(f, S, eps)
            assert at.tolist() == want, (eps, at)
            assert trans[5] == 1 and all(l == sorted(l) for l in lists)
        trans, at, _ = er.march(er.factors(nan, z, 0.02, 1.0, active), S, 1.0)
        assert np.isnan(trans[3]) and at[3] == T  # a NaN compares false: never retired
    # T^ from a full render's weights: exact in float64 for exact weights
    alpha = rng.uniform(0.0, 0.5, (3, T))
    trans = np.cumprod(np.concatenate([np.ones((3, 1)), 1 - alpha], 1), 1)
    assert np.allclose(er.transmittance_from_weights(alpha * trans[:, :-1]), trans, rtol=0, atol=1e-12)


# ---- the scenes, on the CPU oracle ------------------------------------------------------------------------------------------
def _mix(weights, eps):
    """-> {retirement point: rays}, rays never retired (all T samples evaluated), rays left out: T within a factor 2 of eps at a
    slab end, where the oracle's and a kernel's rounding may decide differently."""
    at, near = er.predict_retirement(weights, SLAB, eps, 1.0)
    points, counts = np.unique(at[~near], return_counts=True)
    mix = dict(zip(points.tolist(), counts.tolist()))
    return mix, mix.pop(T_STEPS, 0), int(near.sum())


def test_uniform_scenes_retire_where_expected():
    """density_scale 40 (smoke()'s scene): every ray retires after the same slab, at eps = 5e-5 with no ray near the threshold."""
    out, _ = oracle_render(OPAQUE_SCALE, None)
    mix, never, near = _mix(out["weights"], 5e-5)
    assert mix == {48: N_RAYS} and never == 0 and near == 0, (mix, never, near)
    out, _ = oracle_render(8.0, None)
    mix, never, near = _mix(out["weights"], 5e-5)
    assert mix == {} and never == N_RAYS, (mix, never, near)


@pytest.mark.parametrize("eps", [1e-4, 5e-5])
def test_mixed_scene_has_several_retirement_points(eps):
    """The mixed scene has at least three distinct retirement points with >= 5 rays each and >= 5 rays never retired (all T samples
    evaluated), rays whose T at a slab end lies within a factor 2 of eps counted neither way.

    How G and its density_scale were picked: on a grid of G from -45 to -70 in steps of 5 and density_scale in 1 / 1.5 / 2 / 3 / 5 per
    decade, a pair for which that holds at BOTH eps with room (third point 6 rays, 12 never).  On the oracle (retirement point: rays | never | left out)
    G = -60, density_scale 1e-7:  eps 1e-4: {16: 16, 32: 13, 48: 6, 64: 2, 80: 3} | 12 | 12;  eps 5e-5: {16: 16, 32: 10, 48: 6, 64: 2,
    80: 3} | 13 | 14.  At density_scale 0.5 no gain does: the field has too little contrast there (G = -12: T falls by a factor of 5 to 8
    per slab, three quarters of the rays pass within a factor 2 of eps at a slab end, {64: 4, 80: 8} | 2 | 50 at eps 1e-4; G from -10 to
    -20 in steps of 0.25 never gives three points of five with five rays left over)."""
    out, _ = oracle_render(MIXED_SCALE, G)
    _, near3 = er.predict_retirement(out["weights"], SLAB, eps, 1e-3)
    assert near3.sum() <= 0.05 * N_RAYS  # (what tests/test_gpu_early_stop.py exempts)
    mix, never, near = _mix(out["weights"], eps)
    print("outside a factor 2:", mix, "never", never, "left out", near)
    assert sum(c >= 5 for c in mix.values()) >= 3 and never >= 5, (mix, never, near)


@pytest.mark.parametrize("eps", [1e-4, 5e-5, 1e-2])
@pytest.mark.parametrize("scene", [(MIXED_SCALE, G), (OPAQUE_SCALE, None), SMOOTH, STEEP], ids=["mixed", "opaque", "smooth", "steep"])
def test_zeroing_the_oracles_weights_behind_retirement_stays_inside_the_bound(scene, eps):
    (out, far) = oracle_render(*scene)
    w = out["weights"]
    at, _ = er.predict_retirement(w, SLAB, eps, 0.0)
    culled = er.cull(w, at)
    assert (at < T_STEPS).any() and (culled[:, :SLAB] == w[:, :SLAB]).all()
    z = out["z_vals"].astype(np.float64)
    full = {"weights": w, "weights_sum": w.astype(np.float64).sum(1), "depth": (w * z).sum(1)}
    cut = {"weights": culled, "weights_sum": culled.astype(np.float64).sum(1), "depth": (culled * z).sum(1)}
    er.check_bound(full, cut, eps, far, what=str(scene))
    if eps <= 5e-5:  # no culled sample is in the full render's mask
        assert not (out["mask"] & (culled == 0) & (w != 0)).any()
