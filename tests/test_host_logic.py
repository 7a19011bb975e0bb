"""CPU tests of the host-side logic (no compute calls; the C ABI is tests/test_abi_cpu.py's):
grid geometry agrees with the oracle's, state-dict contract, flat parameter arenas, ray generation against the
reference-generated fixture, the loud failure without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_structs_match_header_layout():
    from lidar4d_amd import _lib
    assert ctypes.sizeof(_lib.GridDesc) == 16 + 4 * 16 * 4
    fd = _lib.FieldDesc
    assert fd.hash_static_table.offset == ctypes.sizeof(_lib.GridDesc)
    assert ctypes.sizeof(_lib.FieldGrads) == 8 * (1 + 24 + 1)


@pytest.mark.parametrize("D,L,F,log2T,base,maxres", [(3, 8, 4, 19, 512, 32768), (2, 8, 4, 15, 512, 32768),
                                                      (3, 8, 8, 18, 32, 8192), (3, 16, 4, 19, 512, 32768),
                                                      (3, 4, 4, 19, 512, 32768), (2, 8, 4, 13, 512, 32768)])
def test_gridmeta_matches_oracle_and_survey(D, L, F, log2T, base, maxres):
    from lidar4d_amd.gridmeta import GridMeta
    from oracle.tcnn_ref import grid_level_meta
    pls = np.exp2(np.log2(maxres / base) / (L - 1))
    m = GridMeta(D, L, F, log2T, base, pls)
    o = grid_level_meta(D, L, log2T, base, pls)
    assert m.res == o["res"] and m.size == o["size"] and m.offset == o["offset"] and m.hashed == o["hashed"]
    assert m.scale == o["scale"]
    if (D, L, base) == (3, 8, 512):
        assert m.res == [512, 928, 1681, 3044, 5513, 9987, 18090, 32768] and all(m.hashed)
        assert m.n_params == 16777216
    if (D, L, base) == (3, 8, 32):
        assert m.res == [32, 71, 157, 345, 761, 1681, 3710, 8192] and m.hashed == [False] + [True] * 7
        assert m.n_params == 14942208


def test_state_dict_contract_and_param_counts():
    from lidar4d_amd import LiDAR4D
    m = LiDAR4D()
    sd = m.state_dict()
    want = {"aabb", "hash_encoder.hash_static.params", "view_encoder.params", "flow_net.grid_enc.params",
            "flow_net.mlp.0.weight", "flow_net.mlp.2.weight", "flow_net.mlp.4.weight", "sigma_net.params",
            "intensity_net.params", "raydrop_net.params"}
    want |= {f"planes_encoder.planes.{s}.{c}" for s in range(4) for c in range(6)}
    want |= {f"hash_encoder.hash_dynamic.{p}.hash_t.{k}.params" for p in range(3) for k in range(8)}
    unet_keys = set(np.load(os.path.join(os.path.dirname(__file__), "golden", "unet_eval.npz"))["keys"])
    want |= {"unet." + k for k in unet_keys}  # lidar4d.py:119; key list recorded from the reference's UNet
    assert set(sd.keys()) == want
    assert tuple(sd["planes_encoder.planes.3.0"].shape) == (1, 8, 256, 256)
    assert tuple(sd["planes_encoder.planes.1.2"].shape) == (1, 8, 8, 64)  # time plane: [1,8,8,R]
    assert sd["hash_encoder.hash_static.params"].numel() == 16777216
    assert sd["hash_encoder.hash_dynamic.0.hash_t.0.params"].numel() == 1048576
    assert sd["hash_encoder.hash_dynamic.1.hash_t.7.params"].numel() == 262144
    assert sd["flow_net.grid_enc.params"].numel() == 14942208
    assert sd["sigma_net.params"].numel() == 9216 and sd["intensity_net.params"].numel() == 11264
    assert tuple(sd["flow_net.mlp.4.weight"].shape) == (6, 64) and sd["view_encoder.params"].numel() == 0
    n = sum(p.numel() for k, p in m.named_parameters() if not k.startswith("unet."))
    assert n == 2181120 + 16777216 + 12582912 + 14942208 + 5504 + 31744
    # optimizer groups as lidar4d.py:226-237
    groups = m.get_params(1e-2)
    assert [g["lr"] for g in groups] == [1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 1e-3, 1e-3]
    assert sum(p.numel() for g in groups for p in g["params"]) == n


def test_param_store_views_and_reload():
    from lidar4d_amd import LiDAR4D
    from oracle.detparams import fill_model
    from oracle.make_golden import SMALL_MODEL
    m = LiDAR4D(**SMALL_MODEL)
    st = m._store
    base = st.flat.data_ptr()
    for _, p, off, n, _ in st.entries:
        if n:
            assert p.data_ptr() == base + 4 * off and off % 8 == 0
    # the flow MLP's [6,64] output layer owns a zero-padded [16,64] slot read by the MFMA kernel
    w = m.flow_net.linears()
    o0 = st.by_param[id(w[0].weight)][0]
    assert st.by_param[id(w[1].weight)][0] == o0 + 1024 and st.by_param[id(w[2].weight)][0] == o0 + 1024 + 4096
    assert float(st.flat[o0 + 5120 + 384: o0 + 6144].abs().sum()) == 0.0
    fill_model(m, seed=3)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m2 = LiDAR4D(**SMALL_MODEL)
    m2.load_state_dict(sd)
    assert torch.equal(m2._store.flat, m._store.flat)  # load_state_dict writes through the views
    g = st.prepare_grads()
    assert m.sigma_net.params.grad.data_ptr() == g.data_ptr() + 4 * st.by_param[id(m.sigma_net.params)][0]
    m.sigma_net.params.grad.fill_(2.0)
    assert float(st.grad_view(m.sigma_net.params).sum()) == 2.0 * m.sigma_net.params.numel()
    m.zero_grad(set_to_none=False)
    assert float(st.flat_grad.abs().sum()) == 0.0


def test_get_lidar_rays_matches_reference_fixture(golden):
    from lidar4d_amd.data import get_lidar_rays
    g = golden("rays_64x1024")
    r = get_lidar_rays(torch.from_numpy(g["poses"]), tuple(g["fov"]), int(g["H"]), int(g["W"]), -1)
    sel = torch.from_numpy(g["sel"])
    assert torch.allclose(r["rays_d"][:, sel], torch.from_numpy(g["rays_d"]), rtol=0, atol=1e-6)
    assert torch.allclose(r["rays_o"][:, sel], torch.from_numpy(g["rays_o"]), rtol=0, atol=0)
    assert np.allclose(r["rays_d"].double().abs().sum(1).numpy(), g["rays_d_abs_sum"], rtol=1e-6)


def test_synthetic_dataset_contract():
    from lidar4d_amd.data import SyntheticKitti360
    ds = SyntheticKitti360("cpu", H=16, W=64, num_frames=5, num_rays=100)
    b = ds.batch()
    assert set(b) >= {"rays_o_lidar", "rays_d_lidar", "time", "images_lidar", "poses_lidar", "H_lidar", "W_lidar"}
    assert b["rays_o_lidar"].shape == (1, 100, 3) and b["images_lidar"].shape == (1, 100, 3) and b["time"].shape == (1, 1)
    assert float((b["rays_d_lidar"].norm(dim=-1) - 1).abs().max()) < 1e-5
    img = ds.images
    assert set(img[..., 0].unique().tolist()) <= {0.0, 1.0} and float(img[..., 1].max()) <= 1.0
    assert 0 < float(img[..., 2].max()) < 81 * ds.scale


def test_no_cpu_fallback():
    from lidar4d_amd import LiDAR4D, _lib
    from oracle.make_golden import SMALL_MODEL
    m = LiDAR4D(**SMALL_MODEL)
    with pytest.raises(_lib.HipExtensionError):
        m.render(torch.zeros(1, 4, 3), torch.ones(1, 4, 3), torch.tensor([[0.3]]))
    with pytest.raises(_lib.HipExtensionError):
        m.density(torch.zeros(4, 3), torch.tensor([[0.3]]))


def test_product_does_not_import_oracle():
    import subprocess
    import sys
    code = "import sys; import lidar4d_amd, lidar4d_amd.trainer, lidar4d_amd.data; assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'product imports oracle'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    for root, _, files in os.walk(os.path.join(ROOT, "lidar4d_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f


def test_raydrop_meter_formulas():
    """lidar4d_amd.metrics.RaydropMeter against the reference's numpy formulas (utils/metrics.py:190-214), restated here."""
    from lidar4d_amd.metrics import RaydropMeter
    rng = np.random.default_rng(0)
    m = RaydropMeter()
    want = []
    for _ in range(3):
        preds = rng.random((1, 16, 64)).astype(np.float32)
        truths = (rng.random((1, 16, 64)) > 0.3).astype(np.float32)
        m.update(torch.from_numpy(preds), torch.from_numpy(truths))
        rmse = np.sqrt(((truths - preds) ** 2).mean())
        mask = np.where(preds > 0.5, 1, 0)
        acc = (mask == truths).mean()
        tp, fp = np.sum((truths == 1) & (mask == 1)), np.sum((truths == 0) & (mask == 1))
        fn = np.sum((truths == 1) & (mask == 0))
        p, r = tp / (tp + fp), tp / (tp + fn)
        want.append([rmse, acc, 2 * p * r / (p + r)])
    np.testing.assert_allclose(m.measure(), np.array(want).mean(0), rtol=1e-6)
    assert "Rdrop_error" in m.report()
    m.clear()
    assert m.N == 0 and m.V == []


class _OracleChamfer:
    """chamfer_3DDist stand-in for CPU tests: the oracle's brute force (the product's operator is HIP-only)."""

    def __call__(self, a, b):
        from oracle import chamfer_ref
        return chamfer_ref.chamfer(a, b)


def _train_cases():
    from tests import train_golden
    return train_golden.cases()


@pytest.mark.parametrize("tag", ["default", "flow_mid", "flow_first", "flow_last", "urf", "crit_huber_bce_l1", "crit_mse_l1_huber", "patch_l1",
                                 "patch_sobel_cos_all", "patch_mse_tv", "everything"])
def test_training_losses_vs_reference_train_step(tag, monkeypatch):
    """lidar4d_amd.trainer's loss terms against the loss block of the REFERENCE's own Trainer.train_step
    (model/runner.py:179-367, run by oracle/make_golden_train.py on seeded tensors): value and d(loss) / d(every render and flow
    output), for the default criteria, the other criterion choices of main_lidar4d.py:183-196, the scene-flow term at a middle /
    first / last frame, the line-of-sight term and the patch-gradient terms with all their switches."""
    from tests import train_golden
    import lidar4d_amd.chamfer as chamfer_mod
    assert tag in train_golden.cases()
    monkeypatch.setattr(chamfer_mod, "chamfer_3DDist", _OracleChamfer)
    c = train_golden.load(tag)
    assert bool(c["render_perturb"]) and not bool(c["render_staged"])  # what the training render call must pass (runner.py:183-191)
    loss, leaves = train_golden.evaluate(c)
    train_golden.check(c, loss, leaves)


@pytest.mark.parametrize("tag", ["default", "flow_mid", "flow_first", "flow_last", "urf", "crit_huber_bce_l1", "patch_l1"])
def test_trainer_compute_loss_vs_reference_train_step(tag, monkeypatch):
    """The same fixture through Trainer.compute_loss (how the terms are COMBINED: which are on, the frame index, the ground
    points' random time, the 1 / world factors at world = 1), for the option sets compute_loss exposes."""
    from tests import train_golden
    import lidar4d_amd.chamfer as chamfer_mod
    monkeypatch.setattr(chamfer_mod, "chamfer_3DDist", _OracleChamfer)
    c = train_golden.load(tag)
    loss, leaves = train_golden.evaluate(c, compute_loss=True)
    train_golden.check(c, loss, leaves)


def test_flat_ema_matches_torch_ema_rule():
    """trainer.FlatEMA against torch_ema's update rule applied tensor by tensor (runner.py:97-98,534-535,565-567)."""
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.trainer import FlatEMA
    from oracle.make_golden import SMALL_MODEL
    m = LiDAR4D(**SMALL_MODEL)
    params = [p for _, p, _, n, _ in m._store.entries]
    shadow = [p.detach().clone() for p in params]
    ema = FlatEMA(m, decay=0.95)
    g = torch.Generator().manual_seed(1)
    for t in range(1, 5):
        with torch.no_grad():
            m._store.flat.add_(torch.randn(m._store.numel, generator=g) * 0.01)
        ema.update()
        decay = min(0.95, (1 + t) / (10 + t))
        for s_, p in zip(shadow, params):
            s_.sub_((1 - decay) * (s_ - p.detach()))
    for s_, v in zip(shadow, ema._views(ema.shadow)):
        assert torch.allclose(s_, v, rtol=1e-5, atol=1e-7)
    live = m._store.flat.clone()
    ema.store()
    ema.copy_to()
    assert torch.equal(m._store.flat, ema.shadow) and torch.equal(params[0].detach().reshape(-1), ema.shadow[: params[0].numel()])
    ema.restore()
    assert torch.equal(m._store.flat, live)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow_params", "collected_params"} and sd["num_updates"] == 4
    other = FlatEMA(m, decay=0.5)
    other.load_state_dict(sd)
    assert other.decay == 0.95  # (alignment gaps of the arena are not parameters: compare the views)
    assert all(torch.equal(a, b) for a, b in zip(other._views(other.shadow), ema._views(ema.shadow)))


def test_flat_adam_state_dict_interchange_with_torch_adam():
    """FlatAdam.state_dict()/load_state_dict() speak torch.optim.Adam's format for LiDAR4D.get_params (what the reference's
    checkpoints hold under "optimizer", runner.py:966,1056-1059)."""
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.trainer import FlatAdam
    from oracle.make_golden import SMALL_MODEL
    m = LiDAR4D(**SMALL_MODEL)
    ref_opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):  # real torch.optim.Adam steps on CPU build a genuine state
        for p in m.parameters():
            if p.numel() and not any(p is q for q in m.unet.parameters()):
                p.grad = torch.randn(p.shape, generator=g) * 1e-3
        ref_opt.step()
    sd = ref_opt.state_dict()
    fa = FlatAdam(m, lr=1e-2)
    fa.load_state_dict(sd)
    assert fa.step_count == 3
    for k, st in sd["state"].items():
        p = [q for grp in ref_opt.param_groups for q in grp["params"]][k]
        off, n = m._store.by_param[id(p)]
        assert torch.equal(fa.exp_avg[off:off + n], st["exp_avg"].reshape(-1))
        assert torch.equal(fa.exp_avg_sq[off:off + n], st["exp_avg_sq"].reshape(-1))
    # and back: a fresh torch optimiser accepts FlatAdam's state and holds the same moments
    out = fa.state_dict()
    assert [len(g_["params"]) for g_ in out["param_groups"]] == [len(g_["params"]) for g_ in sd["param_groups"]]
    fresh = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    fresh.load_state_dict(out)
    for k, st in sd["state"].items():
        p = [q for grp in fresh.param_groups for q in grp["params"]][k]
        assert torch.equal(fresh.state[p]["exp_avg"], st["exp_avg"]) and float(fresh.state[p]["step"]) == 3.0
    assert abs(fresh.param_groups[3]["lr"] - 0.1 * fa.lr()) < 1e-12 and abs(fresh.param_groups[0]["lr"] - fa.lr()) < 1e-12


def test_parameter_order_equals_reference():
    """Positional checkpoint formats (torch.optim state, torch_ema shadow lists) need the reference's registration order."""
    from lidar4d_amd import LiDAR4D
    from oracle.make_golden import SMALL_MODEL
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "param_order.npz"))
    m = LiDAR4D(**SMALL_MODEL)
    assert [n for n, _ in m.named_parameters()] == list(g["names"])
    assert list(m.state_dict().keys()) == list(g["state_keys"])


def test_checkpoint_roundtrip_and_reference_style_file(tmp_path):
    """lidar4d_amd.checkpoint: the reference's checkpoint layout (runner.py:955-1075) out and in, including a file put
    together the way the reference's Trainer does (torch.optim.Adam state, torch_ema-style shadow list, bare state dict)."""
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.checkpoint import latest_checkpoint, load_checkpoint, save_checkpoint
    from lidar4d_amd.trainer import FlatAdam, FlatEMA
    from oracle.detparams import fill_model
    from oracle.make_golden import SMALL_MODEL
    m = fill_model(LiDAR4D(**SMALL_MODEL), seed=4)
    opt, ema = FlatAdam(m, lr=1e-2, iters=100), FlatEMA(m, 0.95)
    opt.step_count = 7
    # per-range step counts as a real run leaves them: time-slice tables that were rarely selected lag behind (the reference's
    # torch.optim.Adam skips tensors whose .grad is None), one was never touched at all
    opt.steps.fill_(7)
    gated = [r for r, g in enumerate(opt.ranges.gate_idx) if g >= 0]
    assert len(gated) == 3 * 8
    opt.steps[gated[1]] = 3
    opt.steps[gated[2]] = 0
    opt.exp_avg.normal_(generator=torch.Generator().manual_seed(1))
    opt.exp_avg_sq.uniform_(generator=torch.Generator().manual_seed(2))
    ema.shadow.mul_(0.5)
    ema.num_updates = 7
    path = save_checkpoint(str(tmp_path / "ckpt" / "run_ep0003.pth"), m, opt, ema, epoch=3, global_step=7)
    assert latest_checkpoint(str(tmp_path / "ckpt"), "run") == path
    raw = torch.load(path, weights_only=False)
    assert set(raw) == {"epoch", "global_step", "stats", "optimizer", "lr_scheduler", "scaler", "ema", "model"}
    assert raw["lr_scheduler"]["last_epoch"] == 7 and len(raw["ema"]["shadow_params"]) == len(list(m.parameters()))
    # a torch optimiser + LambdaLR accept what was written (this is what the reference's Trainer.load_checkpoint does)
    t_opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    t_opt.load_state_dict(raw["optimizer"])
    sched = torch.optim.lr_scheduler.LambdaLR(t_opt, lambda it: 0.1 ** min(it / 100, 1))
    sched.load_state_dict(raw["lr_scheduler"])
    assert sched.last_epoch == 7
    # load into a differently initialised model
    m2 = fill_model(LiDAR4D(**SMALL_MODEL), seed=9)
    opt2, ema2 = FlatAdam(m2, lr=1e-2, iters=100), FlatEMA(m2, 0.5)
    info = load_checkpoint(path, m2, opt2, ema2)
    assert info["epoch"] == 3 and info["global_step"] == 7 and not info["missing_keys"] and not info["unexpected_keys"]
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert opt2.step_count == 7 and ema2.decay == 0.95 and ema2.num_updates == 7
    assert torch.equal(opt2.steps, opt.steps)  # differing per-parameter step counts survive the round trip
    steps_written = sorted({int(v["step"]) for v in raw["optimizer"]["state"].values()})
    assert steps_written == [3, 7]
    for (_, p, off, n, _), (_, p2, off2, _, _) in zip(m._store.entries, m2._store.entries):
        if int(opt.steps[opt._range_of[id(p)]]) == 0:
            continue  # never stepped: no optimiser state is written for it, as in torch
        assert torch.equal(opt.exp_avg[off:off + n], opt2.exp_avg[off2:off2 + n])
        assert torch.equal(ema.shadow[off:off + n], ema2.shadow[off2:off2 + n])
    # bare state dict (runner.py:1027-1030) and model_only
    torch.save(m.state_dict(), str(tmp_path / "bare.pth"))
    m3 = fill_model(LiDAR4D(**SMALL_MODEL), seed=5)
    load_checkpoint(str(tmp_path / "bare.pth"), m3)
    assert torch.equal(m3._store.flat, m._store.flat) or all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m3.state_dict().values()))
    opt4 = FlatAdam(m3, lr=1e-2)
    load_checkpoint(path, m3, opt4, model_only=True)
    assert opt4.step_count == 0


def test_shift_trajectory_matches_reference_script():
    """simulator.shift_trajectory against a transcription of main_lidar4d_sim.py:249-275."""
    import torch.nn.functional as F
    from lidar4d_amd.simulator import shift_trajectory
    g = torch.Generator().manual_seed(3)
    origins = torch.cumsum(torch.rand(6, 1, 3, generator=g) * 0.02, dim=0)
    rays_o = origins.expand(6, 5, 3).contiguous()
    for align in (False, True):
        sx, sy, sz, scale = 1.5, -0.7, 0.3, 0.0105
        want = rays_o.clone()
        shift_x, shift_y = sx, sy
        forward = torch.tensor([[1, 0, 0]]).to(rays_o)
        for i in range(rays_o.shape[0]):
            if align:
                if i < rays_o.shape[0] - 1:
                    forward = F.normalize((rays_o[i + 1, 0, :] - rays_o[i, 0, :]).unsqueeze(0), p=2)
                left = torch.tensor([-forward[:, 1], forward[:, 0], forward[:, 2]]).to(forward)
                shift_x = (sx * forward + sy * left)[:, 0]
                shift_y = (sx * forward + sy * left)[:, 1]
            want[i, :, 0] = want[i, :, 0] + shift_x * scale
            want[i, :, 1] = want[i, :, 1] + shift_y * scale
            want[i, :, 2] = want[i, :, 2] + sz * scale
        got = shift_trajectory(rays_o, sx, sy, sz, scale, align_axis=align)
        assert torch.allclose(got, want, rtol=0, atol=1e-7), align


def test_simulator_pipeline_with_stub_model(tmp_path):
    """Simulator.render's frame loop (simulator.py:104-195): staged render -> U-Net -> mask -> range image to points ->
    files, with a stub model and the numpy conversion standing in for the device parts (each of which has its own GPU
    parity test); what is under test is the glue."""
    import types
    from lidar4d_amd.simulator import Simulator
    from oracle import convert_ref
    H, W = 8, 32

    class Stub:
        calls = []

        def render(self, rays_o, rays_d, time, staged=False, perturb=True, **kw):
            Stub.calls.append((tuple(rays_o.shape), staged, perturb, kw.get("num_steps")))
            n = rays_o.shape[1]
            depth = (torch.arange(n, dtype=torch.float32).view(1, n) % 7 + 1) * 0.05 + float(time)
            drop = (torch.arange(n).view(1, n) % 3 != 0).float()
            return {"depth_lidar": depth, "image_lidar": torch.stack([drop, torch.full((1, n), 0.25)], -1)}

        def unet(self, x):  # [1, 3, H, W] -> [1, 1, H, W]: pass the ray-drop channel through, but drop the first row
            out = x[:, :1].clone()
            out[:, :, 0] = 0.0
            return out

    opt = types.SimpleNamespace(scale=0.01, fov_lidar=[2.0, 26.9], num_steps=64)
    to_points = lambda d, i, fov: convert_ref.pano_to_lidar_with_intensities(d.numpy().astype(np.float32), i.numpy().astype(np.float32), fov)
    sim = Simulator("stub", opt, Stub(), device="cpu", mute=True, workspace=str(tmp_path), use_checkpoint="scratch",
                    H_lidar=H, W_lidar=W, to_points=to_points)
    frames = 3
    rays_o, rays_d = torch.zeros(frames, H * W, 3), torch.zeros(frames, H * W, 3)
    times = torch.tensor([[0.0], [0.5], [1.0]])
    last = sim.render(rays_o, rays_d, times)
    assert Stub.calls == [((1, H * W, 3), True, False, 64)] * frames
    for i in range(frames):
        pts = np.load(tmp_path / "points" / f"lidar4d_{i:04d}.npy")
        keep = (np.arange(H * W) % 3 != 0).reshape(H, W)
        keep[0] = False  # the stub U-Net vetoes the first row
        assert pts.shape == (int(keep.sum()), 4) and np.all(pts[:, 3] == 0.25)
        rng = np.linalg.norm(pts[:, :3], axis=1)
        want = (((np.arange(H * W) % 7 + 1) * 0.05 + float(times[i])) / 0.01).reshape(H, W)[keep]
        np.testing.assert_allclose(rng, want, rtol=1e-5)
    assert np.array_equal(last, np.load(tmp_path / "points" / f"lidar4d_{frames - 1:04d}.npy"))
    assert os.path.exists(tmp_path / "images" / "lidar4d_0000.png") and os.path.exists(tmp_path / "log_stub.txt")


def test_refine_unet_loop_learns_and_follows_reference_recipe():
    """trainer.refine_unet (runner.py:865-912: BCE, Adam 1e-3 under OneCycleLR, random blank boxes) on a toy problem; the
    U-Net is a plain torch module, so this runs on CPU."""
    from lidar4d_amd.trainer import refine_unet
    from lidar4d_amd.unet import UNet
    torch.manual_seed(0)
    net = UNet(in_channels=3, out_channels=1)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 32, 64, generator=g)
    gt = (x[:, :1] > 0.5).float()  # learnable: threshold of the first channel
    calls = []
    rs = np.random.RandomState(3)
    losses = refine_unet(net, x, gt, epochs=40, rng=rs, log=calls.append)
    assert len(losses) == 40 and all(np.isfinite(losses)) and np.mean(losses[-5:]) < 0.85 * np.mean(losses[:5])
    assert not net.training and len(calls) == 1 and calls[0].startswith("iter:0, lr:")
    # the box recipe consumes the numpy stream like the reference: count, then (height, width, top, left) per box
    rs2 = np.random.RandomState(3)
    n_boxes = rs2.randint(32)
    first = (rs2.randint(1, 3), rs2.randint(1, 6), None)
    assert 0 <= n_boxes < 32 and 1 <= first[0] < 3 and 1 <= first[1] < 6
    # batch_size picks distinct frames
    losses_b = refine_unet(net, x, gt, epochs=3, batch_size=1, rng=np.random.default_rng(1))
    assert len(losses_b) == 3


def test_frame_index_is_the_fp32_product_of_the_reference():
    """runner.py:228 / lidar4d.py:143: ``int(time * (num_frames - 1))`` with ``time`` an fp32 tensor.  The float64 product of
    the same numbers truncates to k - 1 for about half of the default frame times k / 50."""
    from lidar4d_amd.trainer import frame_index
    wrong64 = 0
    for F in (51, 5, 2, 17, 100, 201):
        for k in range(F):
            t = torch.tensor([[k / (F - 1)]], dtype=torch.float32)
            want = int(t * (F - 1))
            assert frame_index(t, F) == want == int(np.float32(float(t)) * np.float32(F - 1)), (F, k)
            assert frame_index(float(t), F) == want
            if F == 51:
                assert want == k
                wrong64 += int(float(t) * (F - 1)) != k
    assert wrong64 > 20  # what the float64 evaluation would have got wrong


def test_lidar_loss_rejects_unknown_criteria():
    from lidar4d_amd.trainer import lidar_loss
    out = {"image_lidar": torch.rand(1, 4, 2), "depth_lidar": torch.rand(1, 4)}
    with pytest.raises(ValueError):
        lidar_loss(out, torch.rand(1, 4, 3), depth_loss="l3")


def test_flat_adam_ranges_partition_the_arena():
    """FlatAdam cuts the arena into one range per HashGridT time-slice table (gated by its slice index) and one merged range
    per remaining run of an lr group: disjoint, ordered, covering every parameter."""
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.trainer import FlatAdam
    from oracle.make_golden import SMALL_MODEL
    m = LiDAR4D(**SMALL_MODEL)
    opt = FlatAdam(m)
    R, st = opt.ranges, m._store
    assert R.offs[0] == 0 and all(o % 8 == 0 for o in R.offs)
    assert all(R.offs[i] + R.lens[i] == R.offs[i + 1] for i in range(R.n - 1)) and R.offs[-1] + R.lens[-1] == st.numel
    assert sorted(g for g in R.gate_idx if g >= 0) == sorted(list(range(8)) * 3) and R.gate_idx.count(-1) == R.n - 24
    for name, p, off, n, gi in st.entries:
        r = opt._range_of[id(p)]
        assert R.offs[r] <= off and off + n <= R.offs[r] + R.lens[r]
        assert R.lr_mults[r] == (1.0, 0.1)[gi]
        assert (R.gate_idx[r] >= 0) == (".hash_t." in name)
    assert st.grad_numel == st.numel + 32


def test_library_issues_no_memset_or_memcpy_nodes():
    """Graph safety: the library initialises memory and moves single words with KERNELS
    (csrc/common.h l4d_fill_async / l4d_copy_words_async), never with hipMemsetAsync / hipMemcpyAsync -- memset nodes made captured
    training steps fault or go wrong from their second replay on (ROCm 7.2).  Source-level guard; the behaviour itself is
    tests/test_gpu_optim.py::test_graph_replay_equals_eager_step."""
    import glob
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidar4d_amd")
    offenders = []
    for path in sorted(glob.glob(os.path.join(root, "csrc", "*"))):
        if not path.endswith((".hip", ".cpp", ".h")):
            continue
        code = re.sub(r"//[^\n]*", "", open(path).read())          # comments may name the calls
        code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
        if re.search(r"\bhipMem(set|cpy)\w*\s*\(", code):
            offenders.append(os.path.basename(path))
    assert not offenders, offenders
    # and the step's value-carrying reductions go through the library (torch's multi-block reduce carries a memset node)
    for mod in ("fused.py", "flow_field.py"):
        src = open(os.path.join(root, mod)).read()
        assert not re.search(r"\.abs\(\)\.(a?max)\(", src), mod


def test_lidar4d_rejects_hash_encoder_options_the_fused_pipeline_lacks():
    """HashGridT / HashGrid4D accept feature widths 2 / 4 / 8 and other reductions at operator level, the fused render
    pipeline is built for the reference model's own layout (lidar4d.py:51-57: F = 4, four bases, concat, decompose) -- anything
    else must fail in the constructor with a clear message, not later inside the C layer."""
    from lidar4d_amd import LiDAR4D
    LiDAR4D(n_levels_hash=4, log2_hashmap_size=10)  # the supported layout at a small size constructs
    with pytest.raises(ValueError, match="fused pipeline"):
        LiDAR4D(n_levels_hash=4, log2_hashmap_size=10, n_features_per_level_hash=8)


def test_flat_adam_device_schedule_follows_loaded_state():
    """once the learning-rate schedule lives on the device (FlatAdam.device_schedule: [iterations, factor]), loading an
    optimiser state must move it along with the host-side iteration count."""
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.trainer import FlatAdam
    m = LiDAR4D(n_levels_hash=4, log2_hashmap_size=10)
    opt = FlatAdam(m, lr=1e-2, iters=1000)
    sched = opt.device_schedule()
    assert float(sched[0]) == 0.0
    sd = opt.state_dict()
    assert not sd["state"]  # (no step taken yet: torch.optim.Adam has no per-parameter state either)
    for k, (_, prm) in enumerate(opt._torch_layout()):
        if prm.numel() and id(prm) in opt.store.by_param:
            sd["state"][k] = {"step": torch.tensor(250.0), "exp_avg": torch.zeros_like(prm), "exp_avg_sq": torch.zeros_like(prm)}
    opt.load_state_dict(sd)
    assert opt.step_count == 250 and float(opt.sched[0]) == 250.0
    assert abs(float(opt.sched[1]) - 0.1 ** 0.25) < 1e-6
    opt.step_count = 500
    opt.sync_device_schedule()
    assert float(opt.sched[0]) == 500.0


def test_resolve_knobs_tool(tmp_path):
    """tools/resolve_knobs.py (the unifdef that fixed round 4's compile-time knobs at their measured values): resolved branches are
    replaced by the selected side, default blocks of resolved macros disappear, --plain macros lose their guard, unknown conditions
    pass through untouched."""
    import subprocess
    import sys
    src = tmp_path / "k.hip"
    src.write_text("\n".join([
        "#ifndef A", "#define A 1  // on", "#endif",
        "#ifndef B", "#define B 0", "#endif",
        "#ifndef KEEP", "#define KEEP 64  // tile", "#endif",
        "#if A", "int a_on;", "#else", "int a_off;", "#endif",
        "#if !B", "int b_off;", "#endif",
        "#if B", "int b_on;", "#if A", "int nested;", "#endif", "#endif",
        "#ifdef __HIPCC__", "int dev;", "#endif",
        "#ifdef GONE", "int gone;", "#else", "int not_gone;", "#endif",
        "#if A >= 2", "int a2;", "#endif", "int tail;"]))
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resolve_knobs.py"), str(src), "A=1", "B=0", "GONE=", "--plain", "KEEP"], check=True)
    out = src.read_text()
    assert "int a_on;" in out and "a_off" not in out and "int b_off;" in out and "b_on" not in out and "nested" not in out
    assert "#define KEEP 64  // tile" in out and "#ifndef KEEP" not in out and "#define A" not in out and "#define B" not in out
    assert "#ifdef __HIPCC__" in out and "int dev;" in out and "not_gone" in out and "int gone;" not in out and "a2" not in out and out.rstrip().endswith("int tail;")
    assert out.count("#endif") == 1 and out.count("#if") == 1


def test_shipped_code_reads_two_environment_variables():
    """Which kernels run is decided by the arguments of a call.  The process environment reaches the shipped code in two places:
    L4D_TRACE (csrc/capi.cpp, a diagnostic that changes no result) and L4D_LIB (_lib.py, the path of an ablation build).  Every
    read names its variable as a string literal, so that this list is the whole list."""
    import glob
    csrc = glob.glob(os.path.join(ROOT, "lidar4d_amd", "csrc", "*"))
    assert len(csrc) > 40
    c_literal, c_reads = set(), 0
    for path in csrc:
        text = open(path, errors="replace").read()
        c_reads += len(re.findall(r"\bgetenv\s*\(", text))
        c_literal_here = re.findall(r"\bgetenv\s*\(\s*\"([^\"]*)\"", text)
        c_literal |= set(c_literal_here)
        c_reads -= len(c_literal_here)
    assert c_literal == {"L4D_TRACE"} and c_reads == 0, (c_literal, c_reads)
    py = glob.glob(os.path.join(ROOT, "lidar4d_amd", "*.py"))
    assert len(py) > 30
    py_literal, py_reads = set(), 0
    for path in py:
        text = open(path).read()
        py_reads += len(re.findall(r"\benviron\b|\bgetenv\b", text))
        here = re.findall(r"\bos\.environ(?:\.get\(|\[)\s*[\"']([^\"']*)[\"']|\bos\.getenv\(\s*[\"']([^\"']*)[\"']", text)
        py_literal |= {a or b for a, b in here}
        py_reads -= len(here)
    assert py_literal == {"L4D_LIB"} and py_reads == 0, (py_literal, py_reads)
