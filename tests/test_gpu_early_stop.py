"""GPU tests of early ray termination (``render(..., early_stop=eps, slab=S)``: liblidar4d_march.so, include/lidar4d_march.h,
lidar4d_amd/early_stop.py) against the numpy restatement of its retirement rule and the bound of tests/early_stop_ref.py -- pinned on
the CPU by tests/test_early_stop_cpu.py -- and against the plain render.  Run with ``-m gpu`` on an MI355X.

Shapes: 1, 63 / 64, 65, 257 / 300 and 1100 rays (one wavefront, a tail on either side of a workgroup boundary, several workgroups
with a tail, more than one 1024-ray piece of the ordered compaction); slabs of 16, 32, 96 and 128 samples against 40, 80, 96, 100 and
200 samples per ray (a last slab that is shorter, a slab longer than a wavefront, a slab longer than the ray)."""
import functools
import types

import numpy as np
import pytest
import torch

import early_stop_ref as er
from test_early_stop_cpu import G, MIXED_SCALE, OPAQUE_SCALE, RAY_SEED, TIME, build_scene
from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS7 = ("depth_lidar", "image_lidar", "weights_sum_lidar", "weights", "z_vals", "mask_idx", "mask_count")


def _mask_list(out):
    """The compacted ``weights > 1e-4`` sample indices, ascending (composite_fwd reserves the list's slots per workgroup with an
    atomic: the order of the workgroups' shares differs from launch to launch, the set does not)."""
    return torch.sort(out["mask_idx"][:int(out["mask_count"])]).values


def _bits(t):
    """float32 tensor -> int32 numpy bits, every NaN as one pattern"""
    a = t.detach().float().cpu().numpy().copy()
    a[np.isnan(a)] = np.float32("nan")
    return a.view(np.int32)


# ---- 1. slab_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S", [(96, 32), (100, 32), (96, 128)])
@pytest.mark.parametrize("N", [1, 63, 65, 257])
def test_slab_rows_are_sample_rays_xt_rows(N, T, S):
    from lidar4d_amd import early_stop, ops
    ro, rd = make_rays(N, 11)
    ro, rd = ro.view(-1, 3).to(DEV), rd.view(-1, 3).to(DEV)
    ro = ro + torch.linspace(-0.9, 0.9, N, device=DEV).unsqueeze(1)  # (origins apart, some samples clipped at the bound)
    lin = torch.linspace(0.0, 1.0, T, device=DEV)
    t_dev = torch.tensor([0.37], device=DEV)
    near, far, bound = SMALL_MODEL["near_lidar"], SMALL_MODEL["far_lidar"], 1
    _, full = ops.sample_rays_xt(ro, rd, lin, None, t_dev, near, far, bound)
    full = full.view(N, T, 4)
    lives = {"all": list(range(N)), "third": list(range(0, N, 3)), "one": [N // 2], "empty": []}
    for s0 in list(range(0, T, S)) + [T - 1]:
        Sp = min(S, T - s0)
        for name, rays in lives.items():
            live = torch.tensor(rays + [0] * (N - len(rays)), dtype=torch.int32, device=DEV)  # (the list's buffer is N long)
            got = early_stop.slab_rows(ro, rd, lin, t_dev, live, len(rays), s0, S, near, far, bound)
            want = full[torch.tensor(rays, dtype=torch.long, device=DEV), s0:s0 + Sp].reshape(-1, 4)
            assert got.shape == (len(rays) * Sp, 4) and torch.equal(got, want), (name, s0)


# ---- 2. slab_update on constructed sigma ------------------------------------------------------------------------------------
def _constructed(N, T, S, seed):
    """sigma [N, T], h [N * T, 16], z [N, T].  Ray r by r % 7: opaque in the first slab / the second / the last, thin (never
    retired), all zero (T^ stays exactly 1), an inf in the second slab, a NaN at sample 2 (never retired, whatever follows)."""
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.0, 2.0, (N, T)).astype(np.float32)
    n_slabs = -(-T // S)
    for r in range(N):
        kind = r % 7
        if kind == 0:
            sigma[r, rng.integers(0, S)] = 3e7
        elif kind == 1:
            sigma[r, S + rng.integers(0, min(S, T - S))] = 3e7
        elif kind == 2:
            sigma[r, (n_slabs - 1) * S + rng.integers(0, T - (n_slabs - 1) * S)] = 3e7
        elif kind == 3:
            sigma[r] *= 1e-3
        elif kind == 4:
            sigma[r] = 0.0
        elif kind == 5:
            sigma[r, S + 1] = np.inf
        else:
            sigma[r, 2] = np.nan
            sigma[r, 5] = 3e7
    z = np.sort(rng.uniform(0.01, 0.85, (N, T)).astype(np.float32), axis=1)
    h = rng.standard_normal((N * T, 16)).astype(np.float16)
    return sigma, h, z


def _device_exp(e):
    return torch.exp(torch.from_numpy(np.ascontiguousarray(e)).to(DEV)).cpu().numpy()


def _march_on_device(sigma, h, z, S, sample_dist, density_scale, active, eps):
    from lidar4d_amd import early_stop
    N, T = sigma.shape
    sg, hh, zz = torch.from_numpy(sigma).to(DEV), torch.from_numpy(h).to(DEV), torch.from_numpy(z).to(DEV)
    sigma_dense = torch.full((N, T), 7.0, device=DEV)
    h_dense = torch.full((N * T, 16), 9.0, dtype=torch.float16, device=DEV)
    retired_at = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    trans, live, n_next = early_stop.march_init(N, DEV)
    assert torch.equal(trans, torch.ones(N, device=DEV)) and live.tolist() == list(range(N)) and int(n_next) == N
    live_next = torch.full_like(live, -1)
    lists, n_live, s0 = [], N, 0
    while s0 < T and n_live > 0:
        Sp = min(S, T - s0)
        rows = live[:n_live].long()
        lists.append(rows.tolist())
        sigma_c = sg[rows, s0:s0 + Sp].reshape(-1).contiguous()
        h_c = hh.view(N, T, 16)[rows, s0:s0 + Sp].reshape(-1, 16).contiguous()
        early_stop.slab_update(sigma_c, h_c, zz, live, n_live, s0, S, sample_dist, density_scale, active, eps, trans, sigma_dense, h_dense,
                               retired_at, live_next, n_next)
        n_live, s0 = int(n_next), s0 + Sp
        live, live_next = live_next, live
    torch.cuda.synchronize()
    return trans, sigma_dense, h_dense, retired_at, lists, n_live


@pytest.mark.parametrize("eps", [0.0, 5e-5, 1e-2, 1.0])
@pytest.mark.parametrize("active", [False, True], ids=["passive", "active"])
@pytest.mark.parametrize("N,T,S", [(1, 80, 32), (64, 80, 32), (65, 200, 96), (300, 80, 32), (1100, 40, 16)])
def test_slab_update_against_the_float32_reference(N, T, S, active, eps):
    sigma, h, z = _constructed(N, T, S, seed=N + T)
    sample_dist, density_scale = 0.0123, 1.7
    f = er.factors(sigma, z, sample_dist, density_scale, active, exp=_device_exp)
    want_trans, want_at, want_lists = er.march(f, S, eps)
    got = _march_on_device(sigma, h, z, S, sample_dist, density_scale, active, eps)
    trans, sigma_dense, h_dense, retired_at, lists, n_left = got
    assert lists == want_lists and all(l == sorted(l) for l in lists) and n_left == 0
    assert retired_at.cpu().numpy().tolist() == want_at.tolist()
    assert np.array_equal(_bits(trans), _bits(torch.from_numpy(want_trans))), "trans bits"
    # dense sigma: the values at evaluated samples, zeros behind a retirement; h: the rows at evaluated samples, the rest untouched
    at = want_at
    want_sigma = er.cull(sigma, at)
    assert np.array_equal(_bits(sigma_dense), _bits(torch.from_numpy(want_sigma)))
    hd = h_dense.view(N, T, 16).cpu().numpy()
    hw = h.reshape(N, T, 16)
    for r in range(N):
        assert np.array_equal(hd[r, :at[r]], hw[r, :at[r]]) and (hd[r, at[r]:] == np.float16(9.0)).all(), r
    if eps == 0.0:
        assert (at == T).all()
    if N >= 7:
        kinds = np.arange(N) % 7
        assert (at[kinds == 4] == T).all() and (at[kinds == 6] == T).all()  # all-zero sigma (even at eps = 1), NaN
        if eps > 0:
            assert (at[kinds == 0] == S).all()
        if 0 < eps < 1:  # (at eps = 1 any ray with a non-zero sigma in its first slab is retired after it)
            assert (at[kinds == 1] == min(2 * S, T)).all() and (at[kinds == 5] == min(2 * S, T)).all() and (at[kinds == 3] == T).all()
    # the same bits twice
    again = _march_on_device(sigma, h, z, S, sample_dist, density_scale, active, eps)
    assert np.array_equal(_bits(again[0]), _bits(trans)) and np.array_equal(_bits(again[1]), _bits(sigma_dense))
    assert torch.equal(again[2], h_dense) and torch.equal(again[3], retired_at) and again[4] == lists


# ---- the model ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(density_scale, g):
    from lidar4d_amd import LiDAR4D
    model = build_scene(LiDAR4D, density_scale, g).to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def _rays(N):
    ro, rd = make_rays(N, RAY_SEED)
    return ro.to(DEV), rd.to(DEV), torch.tensor([[TIME]], device=DEV)


@functools.lru_cache(maxsize=None)
def _plain(density_scale, g, N, T):
    """The plain no-grad render of a scene, computed once and shared (not written to)."""
    ro, rd, t = _rays(N)
    with torch.no_grad():
        return _model(density_scale, g).render(ro, rd, t, num_steps=T, perturb=False)


SCENES = [(MIXED_SCALE, G), (OPAQUE_SCALE, None)]


# 3. eps = 0: nothing is ever retired, every output is the plain render's
@pytest.mark.parametrize("N,T,S", [(64, 96, 16), (70, 100, 32)])
@pytest.mark.parametrize("scene", SCENES, ids=["mixed", "opaque"])
def test_eps_zero_equals_the_plain_render(scene, N, T, S):
    model, plain = _model(*scene), _plain(*scene, N, T)
    ro, rd, t = _rays(N)
    with torch.no_grad():
        out = model.render(ro, rd, t, num_steps=T, early_stop=0.0, slab=S)
        staged_plain = model.render(ro, rd, t, num_steps=T, staged=True, max_ray_batch=24)
        staged = model.render(ro, rd, t, num_steps=T, staged=True, max_ray_batch=24, early_stop=0.0, slab=S)
    assert int(out["evaluated_samples"]) == N * T and bool((out["retired_at"] == T).all())
    for k in KEYS7:
        if k == "mask_idx":
            assert torch.equal(_mask_list(out), _mask_list(plain)), k
        else:
            print(k, float((out[k].double() - plain[k].double()).abs().max()))
            assert out[k].shape == plain[k].shape and torch.equal(out[k], plain[k]), k
    for k in ("depth_lidar", "image_lidar"):
        # (against the plain STAGED render: a chunk of 24 rays is below ops.PLANE_ROWS_MIN_POINTS samples and takes the encode's
        # four-tap time planes, the whole batch its 1-D rows, which round differently -- with or without early_stop)
        assert torch.equal(staged[k], staged_plain[k]), ("staged", k)
    assert int(staged["evaluated_samples"]) == N * T and staged["retired_at"].shape == (1, N)


def _np(out, N):
    return {"weights": out["weights"].cpu().numpy(), "weights_sum": out["weights_sum_lidar"].cpu().numpy(),
            "depth": out["depth_lidar"].reshape(N).cpu().numpy(), "image": out["image_lidar"].reshape(N, 2).cpu().numpy()}


# 4. the mixed scene
@pytest.mark.parametrize("N,T,S", [(64, 96, 16), (70, 100, 32)])
def test_mixed_scene_retires_rays_inside_the_bound(N, T, S):
    scene = (MIXED_SCALE, G)
    model, plain = _model(*scene), _plain(*scene, N, T)
    ro, rd, t = _rays(N)
    far = float(model.far_lidar)
    with torch.no_grad():
        out = model.render(ro, rd, t, num_steps=T, early_stop=5e-5, slab=S)
        again = model.render(ro, rd, t, num_steps=T, early_stop=5e-5, slab=S)
        loose = model.render(ro, rd, t, num_steps=T, early_stop=1e-2, slab=S)
    full, got = _np(plain, N), _np(out, N)
    at = out["retired_at"].cpu().numpy()
    assert out["retired_at"].dtype == torch.int32 and out["evaluated_samples"].dtype == torch.int64 and out["evaluated_samples"].is_cuda
    # eps = 5e-5: image and mask list equal, weights equal at evaluated samples and 0 behind, depth / weights_sum inside the bound
    assert torch.equal(out["image_lidar"], plain["image_lidar"])
    assert torch.equal(out["mask_count"], plain["mask_count"]) and torch.equal(_mask_list(out), _mask_list(plain))
    assert np.array_equal(got["weights"], er.cull(full["weights"], at))
    assert torch.equal(out["z_vals"], plain["z_vals"])
    er.check_bound(full, got, 5e-5, far, "eps 5e-5")
    # retired where the plain render's weights say, rays within 1e-3 of eps at a slab end exempt (at most 5 % of the rays)
    want_at, near = er.predict_retirement(full["weights"], S, 5e-5, 1e-3)
    print("retired_at:", dict(zip(*[a.tolist() for a in np.unique(at, return_counts=True)])), "exempt:", int(near.sum()),
          "evaluated:", int(out["evaluated_samples"]), "of", N * T)
    assert near.sum() <= 0.05 * N
    assert np.array_equal(at[~near], want_at[~near]), (at, want_at)
    assert int(out["evaluated_samples"]) == int(at.sum()) < N * T
    assert len(np.unique(at)) >= 2 and (at == T).any() and (at < T).any()
    # eps = 1e-2: the bound for all four outputs
    lo = _np(loose, N)
    er.check_bound(full, lo, 1e-2, far, "eps 1e-2")
    assert np.array_equal(lo["weights"], er.cull(full["weights"], loose["retired_at"].cpu().numpy()))
    assert int(loose["evaluated_samples"]) < int(out["evaluated_samples"])
    # the same bits twice
    for k in KEYS7 + ("retired_at", "evaluated_samples"):
        a, b = (_mask_list(out), _mask_list(again)) if k == "mask_idx" else (out[k], again[k])
        assert torch.equal(a, b), k


# 5. refusals
def test_refusals_on_the_device():
    from lidar4d_amd import LiDAR4D
    model = _model(OPAQUE_SCALE, None)
    ro, rd, t = _rays(8)
    with torch.no_grad():
        with pytest.raises(ValueError, match="perturb=True"):
            model.render(ro, rd, t, num_steps=32, perturb=True, early_stop=1e-4)
        with pytest.raises(ValueError, match="slab must be a positive int"):
            model.render(ro, rd, t, num_steps=32, early_stop=1e-4, slab=0)
        with pytest.raises(ValueError, match="early_stop must be"):
            model.render(ro, rd, t, num_steps=32, early_stop=-1e-4)
        narrow = LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=4, n_levels_plane=4)).to(DEV)
        with pytest.raises(ValueError, match="needs the fused pipeline"):
            narrow.render(ro, rd, t, num_steps=32, early_stop=1e-4)
    trainable = build_scene(LiDAR4D, OPAQUE_SCALE).to(DEV)
    assert torch.is_grad_enabled()
    with pytest.raises(ValueError, match="requires grad"):
        trainable.render(ro, rd, t, num_steps=32, early_stop=1e-4)
    out = model.render(ro, rd, t, num_steps=32, early_stop=1e-4, slab=8)  # grad mode on, nothing requires grad: allowed
    assert not out["depth_lidar"].requires_grad and int(out["evaluated_samples"]) <= 8 * 32


# 6. Simulator and Trainer.test_step
def test_simulator_and_test_step_hand_the_option_on():
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_FOV, KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.simulator import Simulator
    from lidar4d_amd.trainer import Trainer
    from oracle.detparams import fill_model
    torch.manual_seed(0)
    H, W, T = 16, 64, 96
    data = SyntheticKitti360(DEV, H=H, W=W, num_frames=5, num_rays=256)
    cfg = dict(SMALL_MODEL, num_frames=5, near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE, density_scale=OPAQUE_SCALE)
    model = fill_model(LiDAR4D(**cfg), seed=7).to(DEV).eval()
    far, e = float(model.far_lidar), er.eps_prime(5e-5)
    fr = data.frame(2)
    tr = Trainer(model, data, num_steps=T)
    plain = tr.test_step(fr, refine=False, alpha_r=0.0, max_ray_batch=300)
    early = tr.test_step(fr, refine=False, alpha_r=0.0, max_ray_batch=300, early_stop=5e-5, slab=16)
    assert torch.equal(early[0], plain[0]) and torch.equal(early[1], plain[1])  # ray-drop, intensity (before refinement)
    d = float((early[2] - plain[2]).abs().max())
    assert d <= e * far, d
    with torch.no_grad():
        frame = model.render(fr["rays_o_lidar"], fr["rays_d_lidar"], fr["time"], staged=True, max_ray_batch=300, num_steps=T,
                             early_stop=5e-5, slab=16)
    assert int(frame["evaluated_samples"]) == int(frame["retired_at"].sum()) < H * W * T  # (the option did cull)
    seen = {}

    def capture(key):
        def to_points(depth_m, intensity, fov):
            seen[key] = (depth_m.clone(), intensity.clone())
            return depth_m
        return to_points

    opt = types.SimpleNamespace(scale=KITTI360_SCALE, fov_lidar=KITTI360_FOV, num_steps=T, max_ray_batch=300)
    for key, kw in (("plain", {}), ("early", {"early_stop": 5e-5, "slab": 16})):
        sim = Simulator("es", opt, model, device=torch.device(DEV), mute=True, workspace=None, use_refine=False, H_lidar=H, W_lidar=W,
                        to_points=capture(key), **kw)
        sim.render(fr["rays_o_lidar"], fr["rays_d_lidar"], fr["time"], save_pc=False, save_img=False, save_video=False)
    assert torch.equal(seen["early"][1], seen["plain"][1])  # intensity, masked by the (equal) ray-drop
    d = float((seen["early"][0] - seen["plain"][0]).abs().max()) * KITTI360_SCALE
    assert d <= e * far, d
