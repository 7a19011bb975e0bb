"""GPU tests of training on culled samples (``render(..., cull=eps, slab=S)``: lidar4d_amd/cull.py, the work-list mode of
``l4d_sample_rays_xt``) against the plain training render, the numpy restatement and bound of tests/early_stop_ref.py, and the CPU
oracle with its density masked by the device's retirement points.  Run with ``-m gpu`` on an MI355X."""
import numpy as np
import pytest
import torch

import early_stop_ref as er
from test_early_stop_cpu import G, MIXED_SCALE, OPAQUE_SCALE, RAY_SEED, TIME, build_scene
from test_gpu_c3_parity import compare_grads
from oracle import fields_ref, tcnn_ref
from oracle.detparams import det_uniform
from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS7 = ("depth_lidar", "image_lidar", "weights_sum_lidar", "weights", "z_vals", "mask_idx", "mask_count")


def _mask_list(out):
    """The compacted ``weights > 1e-4`` sample indices, ascending (the order of the workgroups' shares differs from launch to launch)."""
    return torch.sort(out["mask_idx"][:int(out["mask_count"])]).values


# ---- 1. rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 96, 200])
@pytest.mark.parametrize("N", [1, 5, 130])
def test_work_list_rows_are_the_dense_rows(N, T):
    """S in 1 / 64 / 96 (one sample, a wavefront, a slab longer than 64 and -- at T = 64 -- than the ray; a partial last slab at T = 96
    and 200), with and without noise; lists: all rays, every third, one, none."""
    from lidar4d_amd import early_stop, ops
    ro, rd = make_rays(N, 11)
    ro, rd = ro.view(-1, 3).to(DEV), rd.view(-1, 3).to(DEV)
    ro = (ro + torch.linspace(-0.9, 0.9, N, device=DEV).unsqueeze(1)).contiguous()  # (origins apart, some samples clipped at the bound)
    lin = torch.linspace(0.0, 1.0, T, device=DEV)
    t_dev = torch.tensor([0.37], device=DEV)
    near, far, bound = SMALL_MODEL["near_lidar"], SMALL_MODEL["far_lidar"], 1
    gen = torch.Generator(device=DEV).manual_seed(100 * N + T)
    lives = {"all": list(range(N)), "third": list(range(0, N, 3)), "one": [N // 2], "empty": []}
    for noise in (None, torch.rand(N, T, device=DEV, generator=gen)):
        z, full = ops.sample_rays_xt(ro, rd, lin, noise, t_dev, near, far, bound)
        # the dense call, new arguments absent: the bits of l4d_sample_rays and the two lines of lidar4d.py:141,148-149 on its points
        z_ref, xyz = ops.sample_rays(ro, rd, lin, noise, near, far, bound, want_xyz=True)
        assert z.shape == (N, T) and full.shape == (N * T, 4)
        assert torch.equal(z, z_ref)
        assert torch.equal(full[:, :3], (xyz + float(bound)) / (2.0 * float(bound))) and bool((full[:, 3] == t_dev).all())
        full = full.view(N, T, 4)
        for S in (1, 64, 96):
            starts = [0, 1, T // 2, T - 1] if S == 1 else sorted(set(list(range(0, T, S)) + [T - 1]))
            for s0 in starts:
                Sp = min(S, T - s0)
                for name, rays in lives.items():
                    live = torch.tensor(rays + [0] * (N - len(rays)), dtype=torch.int32, device=DEV)  # (the list's buffer is N long)
                    got = ops.sample_rays_xt(ro, rd, lin, noise, t_dev, near, far, bound, live=live, n_live=len(rays), s0=s0, S=S)
                    want = full[torch.tensor(rays, dtype=torch.long, device=DEV), s0:s0 + Sp].reshape(-1, 4)
                    assert got.shape == (len(rays) * Sp, 4) and torch.equal(got, want), (name, S, s0, noise is not None)
                    if noise is None and name == "third":  # the inference march's rows are these rows
                        assert torch.equal(got, early_stop.slab_rows(ro, rd, lin, t_dev, live, len(rays), s0, S, near, far, bound))
        # into a caller's buffer at a row offset, nothing written outside the rows
        buf = torch.full((N * T + 8, 4), -7.0, device=DEV)
        live = torch.arange(N, dtype=torch.int32, device=DEV)
        got = ops.sample_rays_xt(ro, rd, lin, noise, t_dev, near, far, bound, live=live, s0=T // 2, S=T, out=buf[4:])
        assert got.data_ptr() == buf[4:].data_ptr() and torch.equal(got, full[:, T // 2:].reshape(-1, 4))
        assert bool((buf[:4] == -7.0).all()) and bool((buf[4 + got.shape[0]:] == -7.0).all())


def test_work_list_argument_checks():
    from lidar4d_amd import ops
    from lidar4d_amd._lib import HipExtensionError
    N, T = 4, 32
    ro, rd = make_rays(N, 11)
    ro, rd = ro.view(-1, 3).to(DEV), rd.view(-1, 3).to(DEV)
    lin = torch.linspace(0.0, 1.0, T, device=DEV)
    t_dev = torch.tensor([0.37], device=DEV)
    live = torch.arange(N, dtype=torch.int32, device=DEV)
    out = torch.full((N * T, 4), -7.0, device=DEV)
    call = lambda **kw: ops.sample_rays_xt(ro, rd, lin, None, t_dev, 0.01, 0.8, 1, live=live, out=out, **kw)
    for kw, text in (({"s0": 0, "S": 0}, "S must be at least 1"), ({"s0": -1, "S": 8}, "s0 outside"), ({"s0": T, "S": 8}, "s0 outside")):
        with pytest.raises(HipExtensionError, match=text):
            call(**kw)
    with pytest.raises(ValueError, match="n_live exceeds"):
        call(n_live=N + 1, s0=0, S=8)
    big = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    with pytest.raises(HipExtensionError, match="n_live outside"):  # (the entry point's own check: more rays listed than there are)
        ops.sample_rays_xt(ro, rd, lin, None, t_dev, 0.01, 0.8, 1, live=big, s0=0, S=1, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # refused calls launch nothing


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _trainable(density_scale, g):
    from lidar4d_amd import LiDAR4D
    return build_scene(LiDAR4D, density_scale, g).to(DEV)


def _rays(N):
    ro, rd = make_rays(N, RAY_SEED)
    return ro.to(DEV), rd.to(DEV), torch.tensor([[TIME]], device=DEV)


def _grads(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()
            if p.numel() and not n.startswith("unet.")}


def _backward(model, out, gd, gi, scale):
    model.zero_grad()
    ((out["depth_lidar"] * gd).sum() + (out["image_lidar"] * gi).sum()).mul(scale).backward()
    return _grads(model)


def _rel_l2(a, b):
    """{name: ||a - b|| / ||b||} over the tensors that have a gradient; the two sides must agree on which have none."""
    out = {}
    for n in b:
        assert (a[n] is None) == (b[n] is None), n
        if b[n] is not None and float(b[n].abs().max()) > 0:
            out[n] = float((a[n].double() - b[n].double()).norm() / b[n].double().norm())
        elif b[n] is not None:
            assert float(a[n].abs().max()) == 0.0, n
    return out


# ---- 2. eps = 0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [37, 48])
@pytest.mark.parametrize("scene", [(MIXED_SCALE, G), (OPAQUE_SCALE, None)], ids=["mixed", "opaque"])
def test_eps_zero_equals_the_plain_training_render(scene, N):
    """N rays x 128 samples, S = 64, jittered.  Every output is the plain training render's; every parameter gradient lies within ten
    times the distance between two plain backward passes of the same inputs, plus 1e-6 (the rows are the same rows: only the order of
    the sums may differ).

    37 rays: 4,736 rows, which the planes' adjoint (csrc/field_bwd.hip) cuts into three chunks of 1,579 -- no multiple of 64, so its
    wavefronts straddle rays and the float run it rounds once to fixed point depends on which rows are neighbours: on slab-major rows
    the hex-plane gradients were 6e-6 .. 4.3e-5 from the plain ones (two plain passes: 0 .. 1e-7), which is why the culled backward
    runs on ray-major rows (cull.py).  48 rays: chunks of 2,048 rows, where the order of the rows does not show."""
    T, S = 128, 64
    model = _trainable(*scene)
    ro, rd, t = _rays(N)
    noise = det_uniform((N, T), "cull2", 0.0, 1.0).to(DEV)
    gd, gi = det_uniform((1, N), "cull2gd", -1, 1).to(DEV), det_uniform((1, N, 2), "cull2gi", -1, 1).to(DEV)
    kw = dict(num_steps=T, perturb=True, noise=noise)
    plain = model.render(ro, rd, t, **kw)
    g_a = _backward(model, plain, gd, gi, 256.0)
    g_b = _backward(model, model.render(ro, rd, t, **kw), gd, gi, 256.0)
    out = model.render(ro, rd, t, cull=0.0, slab=S, **kw)
    assert out["depth_lidar"].requires_grad and out["image_lidar"].requires_grad
    assert int(out["evaluated_samples"]) == N * T and bool((out["retired_at"] == T).all())
    assert out["retired_at"].dtype == torch.int32 and out["evaluated_samples"].dtype == torch.int64 and out["evaluated_samples"].is_cuda
    for k in KEYS7:
        if k == "mask_idx":
            assert torch.equal(_mask_list(out), _mask_list(plain)), k
        else:
            print(k, float((out[k].double() - plain[k].double()).abs().max()))
            assert out[k].shape == plain[k].shape and torch.equal(out[k], plain[k]), k
    g_c = _backward(model, out, gd, gi, 256.0)
    twice, culled = _rel_l2(g_b, g_a), _rel_l2(g_c, g_a)
    assert set(twice) == set(culled) and len(culled) >= 10
    fails = []
    for n in sorted(culled):
        print(f"  {n:48s} plain twice {twice[n]:.3e}   culled vs plain {culled[n]:.3e}")
        if not culled[n] <= 10.0 * twice[n] + 1e-6:
            fails.append((n, twice[n], culled[n]))
    print(f"worst of {len(culled)} tensors (density_scale {scene[0]:g}, {N} rays): plain twice {max(twice.values()):.3e}, "
          f"culled vs plain {max(culled.values()):.3e} ({max(culled, key=culled.get)}); bound missed by {len(fails)}")
    assert not fails, fails


# ---- 3. eps > 0 on the mixed scene -------------------------------------------------------------------------------------------------
def test_mixed_scene_outputs_and_gradients():
    """64 rays x 128 samples of the mixed scene, S = 64, eps = 1e-4, jittered (on the oracle: 44 rays retire after the first slab, 20
    never).  Outputs inside the bound of the plain render; gradients against the oracle whose density is multiplied by the device's M."""
    N, T, S, eps = 64, 128, 64, 1e-4
    prev = tcnn_ref.get_precision()
    tcnn_ref.set_precision("tcnn")
    try:
        ref = build_scene(fields_ref.LiDAR4D, MIXED_SCALE, G)
        hip = _trainable(MIXED_SCALE, G)
        ro, rd, t = _rays(N)
        noise = det_uniform((N, T), "cull3", 0.0, 1.0)
        gd, gi = det_uniform((1, N), "cull3gd", -1, 1), det_uniform((1, N, 2), "cull3gi", -1, 1)
        kw = dict(num_steps=T, perturb=True)
        with torch.no_grad():
            plain = hip.render(ro, rd, t, noise=noise.to(DEV), **kw)
        out = hip.render(ro, rd, t, noise=noise.to(DEV), cull=eps, slab=S, **kw)
        at = out["retired_at"].cpu().numpy()
        w_full = plain["weights"].cpu().numpy()
        # the scene does cull: a quarter of the rays retire before the last slab, and at least one ray never retires
        end = er.transmittance_from_weights(w_full)[:, T]
        print("retired_at:", dict(zip(*[a.tolist() for a in np.unique(at, return_counts=True)])), "never:", int((end >= eps).sum()),
              "evaluated:", int(out["evaluated_samples"]), "of", N * T)
        assert (at < T).sum() >= N / 4 and (end >= 2 * eps).sum() >= 1
        assert set(np.unique(at).tolist()) <= {S, T} and int(out["evaluated_samples"]) == int(at.sum()) < N * T
        want_at, near = er.predict_retirement(w_full, S, eps, 1e-3)
        assert near.sum() <= 0.05 * N
        assert np.array_equal(at[~near], want_at[~near]), (at, want_at)
        assert torch.equal(out["z_vals"], plain["z_vals"])
        np_ = lambda o: {"weights": o["weights"].detach().cpu().numpy(), "weights_sum": o["weights_sum_lidar"].detach().cpu().numpy(),
                         "depth": o["depth_lidar"].detach().reshape(N).cpu().numpy(), "image": o["image_lidar"].detach().reshape(N, 2).cpu().numpy()}
        er.check_bound(np_(plain), np_(out), eps, float(hip.far_lidar), "eps 1e-4")

        # the oracle with sigma * M
        def oracle_backward():
            ref.zero_grad()
            o = ref.render(ro.cpu(), rd.cpu(), t.cpu(), staged=False, noise=noise, **kw)
            ((o["depth_lidar"] * gd).sum() + (o["image_lidar"] * gi).sum()).backward()
            return o

        M = torch.from_numpy(np.arange(T)[None, :] < at[:, None]).reshape(-1)
        density, seen = ref.density, {}

        def masked_density(x, t_):
            seen["x"] = x.detach().clone()
            d = dict(density(x, t_))
            d["sigma"] = d["sigma"] * M.to(d["sigma"].dtype)
            return d

        ref.density = masked_density
        try:
            o_ref = oracle_backward()
        finally:
            del ref.density
        assert torch.equal(out["z_vals"].cpu(), o_ref["z_vals"])
        loss = (out["depth_lidar"] * gd.to(DEV)).sum() + (out["image_lidar"] * gi.to(DEV)).sum()
        scale = 65536.0  # as test_gpu_c3_parity.render_both: GradScaler's initial scale, halved while a gradient overflows
        while True:
            hip.zero_grad()
            (loss * scale).backward(retain_graph=True)
            if bool(torch.isfinite(hip._store.flat_grad).all()):
                break
            scale *= 0.5
            assert scale >= 1.0
        print(f"  loss scale {scale:g}")
        for p in hip.parameters():
            if p.grad is not None:
                p.grad.mul_(1.0 / scale)
        fails = compare_grads(ref, hip)
        assert not fails, fails
        # table entries only culled samples touch -- found from the encoder alone: the gradient of the sum of its features is a sum of
        # positive interpolation weights, non-zero exactly at the touched entries -- have a zero gradient on both sides
        tables = [n for n, _ in ref.named_parameters() if n.startswith("hash_encoder.")]
        named, hip_named = dict(ref.named_parameters()), dict(hip.named_parameters())
        g_ref = {n: None if named[n].grad is None else named[n].grad.detach().clone() for n in tables}

        def touched(x):
            ref.zero_grad()
            feat_s, feat_d = ref.hash_encoder((x + ref.bound) / (2 * ref.bound), torch.tensor([[TIME]]))
            (feat_s.float().sum() + feat_d.float().sum()).backward()
            return {n: named[n].grad.detach() != 0 for n in tables if named[n].grad is not None}

        by_evaluated, by_culled = touched(seen["x"][M]), touched(seen["x"][~M])
        only_culled = 0
        for n in by_culled:
            sel = by_culled[n] & ~by_evaluated[n]
            only_culled += int(sel.sum())
            assert g_ref[n] is not None and float(g_ref[n][sel].abs().sum()) == 0.0, n
            assert hip_named[n].grad is not None and float(hip_named[n].grad.cpu()[sel].abs().sum()) == 0.0, n
        print("  hash-table entries touched by culled samples only:", only_culled)
        assert only_culled > 0
    finally:
        tcnn_ref.set_precision(prev)


# ---- 4. Trainer ---------------------------------------------------------------------------------------------------------------------
def _trainer(**kw):
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.trainer import Trainer
    from oracle.detparams import fill_model
    data = SyntheticKitti360(DEV, H=16, W=64, num_frames=5, num_rays=256, seed=3)
    cfg = dict(SMALL_MODEL, num_frames=5, near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE, density_scale=OPAQUE_SCALE)
    model = fill_model(LiDAR4D(**cfg), seed=7).to(DEV)
    return model, data, Trainer(model, data, num_steps=128, iters=100, chamfer=True, flow=False, init_scale=1024.0, **kw)


def _first_loss(**kw):
    model, data, tr = _trainer(**kw)
    torch.manual_seed(5)
    return float(tr.train_step(data.batch_for(2)))


def test_trainer_steps_on_culled_samples():
    model, data, tr = _trainer(cull=1e-4, cull_slab=64)
    assert tr.graphs_supported() is False
    seen = []
    render = model.render

    def spy(*a, **k):
        out = render(*a, **k)
        seen.append((k.get("cull"), k.get("slab"), out["evaluated_samples"], out["retired_at"]))
        return out

    model.render = spy
    init = model._store.flat.detach().clone()
    b = data.batch_for(2)
    torch.manual_seed(5)
    losses = [float(tr.train_step(b)) for _ in range(3)]
    del model.render
    assert all(np.isfinite(l) for l in losses), losses
    assert [s[:2] for s in seen] == [(1e-4, 64)] * 3
    print("losses", losses, "evaluated", [int(s[2]) for s in seen], "of", 256 * 128)
    assert all(int(s[2]) == int(s[3].sum()) <= 256 * 128 for s in seen)
    assert float((model._store.flat.detach() - init).abs().max()) > 0  # parameters move
    # the frame's time-slice pair was gated open for the optimiser (its tables moved) and no other slice was
    n_slices = model.hash_encoder.hash_dynamic[0].time_resolution
    idx = np.float32(float(b["time"].reshape(-1)[0])) * np.float32(n_slices - 1)
    pair = {int(np.floor(idx)), int(np.ceil(idx))}
    fresh = _trainer()[0]
    for hd, hd0 in zip(model.hash_encoder.hash_dynamic, fresh.hash_encoder.hash_dynamic):
        for s, (enc, enc0) in enumerate(zip(hd.hash_t, hd0.hash_t)):
            assert (not torch.equal(enc.params, enc0.params)) == (s in pair), s
    assert float(model._store.gates[sorted(pair)].abs().min()) > 0  # (raised by the last step's backward, read by its Adam)


def test_trainer_cull_zero_gives_the_plain_first_loss():
    """Same seeds: the first step's loss with ``cull=0.0`` against a trainer without ``cull``, within ten times the distance between
    two trainers without it, plus 1e-6 (test 2's bound)."""
    a, b = _first_loss(), _first_loss()
    c = _first_loss(cull=0.0, cull_slab=64)
    twice, culled = abs(b - a) / abs(a), abs(c - a) / abs(a)
    print(f"first loss {a!r}; plain twice {twice:.3e}, cull=0 vs plain {culled:.3e}")
    assert np.isfinite(c) and culled <= 10.0 * twice + 1e-6, (a, b, c)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(monkeypatch):
    from lidar4d_amd import LiDAR4D, early_stop, ops
    launched = []
    monkeypatch.setattr(ops, "call", lambda name, *a: launched.append(name))
    monkeypatch.setattr(early_stop, "_call", lambda name, *a: launched.append(name))
    model = _trainable(OPAQUE_SCALE, None)
    ro, rd, t = _rays(8)
    for kw, text in ((dict(cull=-1e-4), "cull must be"), (dict(cull=float("nan")), "cull must be"), (dict(cull=True), "cull must be"),
                     (dict(cull=1e-4, slab=0), "slab must be a positive int"), (dict(cull=1e-4, slab=1.5), "slab must be a positive int"),
                     (dict(cull=1e-4, early_stop=1e-4), "cull and early_stop"),
                     (dict(cull=1e-4, staged=True, max_ray_batch=4), "staged=True")):
        with pytest.raises(ValueError, match=text):
            model.render(ro, rd, t, num_steps=32, perturb=True, **kw)
    narrow = LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=4, n_levels_plane=4)).to(DEV)
    with pytest.raises(ValueError, match="cull needs the fused pipeline"):
        narrow.render(ro, rd, t, num_steps=32, cull=1e-4)
    with torch.no_grad(), pytest.raises(ValueError, match="needs a gradient.*early_stop"):
        model.render(ro, rd, t, num_steps=32, cull=1e-4)
    with pytest.raises(ValueError, match="requires grad"):  # early_stop under grad: as before
        model.render(ro, rd, t, num_steps=32, early_stop=1e-4)
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="needs a gradient.*early_stop"):
        model.render(ro, rd, t, num_steps=32, cull=1e-4)
    assert launched == [], launched
