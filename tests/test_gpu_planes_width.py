"""GPU tests of the hex-plane widths 4 and 16 (liblidar4d_planes.so, include/lidar4d_planes.h; Planes4D, Planes4D.density_features,
LiDAR4D without the fused pipeline, one Trainer step) against the float64 yardstick of tests/planes_width_ref.py -- pinned on the
CPU by tests/test_planes_width_cpu.py --, against the width-8 kernels of liblidar4d_hip.so, and against oracle/fields_ref.py in
tiny-cuda-nn rounding mode.  Run with ``-m gpu`` on an MI355X.

Shapes: planes of resolution (8, 12, 16, 5) -- every axis different, the time axis the shortest --, one scale and three
(1, 2, 4); 1, 255, 257 and 4097 samples (one thread, a tail block on either side of a block boundary, more than one block with a
tail).  Coordinates reach a little beyond [0, 1], with fixed rows at exactly 0 and 1, on texel centres, at -0.25 and 1.25, and a
flow of up to 0.3 that takes warped points out of [0, 1].

Bounds: the ones tests/test_gpu_ops.py::test_planes_vs_reference_golden uses for width 8: 2e-5 relative + 1e-6 absolute on values,
1e-4 + 1e-4 on gradients, no element out of tolerance."""
import functools

import numpy as np
import pytest
import torch

import planes_width_ref as pw
from oracle import fields_ref, tcnn_ref
from oracle.detparams import det_uniform, fill_model, grad_digest
from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [((1,), 1), ((1, 2, 4), 255), ((1,), 257), ((1, 2, 4), 4097)]
SHAPE_IDS = ["s1-P1", "s3-P255", "s1-P257", "s3-P4097"]
CFG4 = dict(SMALL_MODEL, n_features_per_level_plane=4, n_levels_plane=4)  # 60 -> 64 columns
CFG16 = dict(SMALL_MODEL, n_features_per_level_plane=16)                  # 92 -> 96 columns


def rel_close(got, ref, rtol, atol, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max abs err {float(err.max()):.3e}, ref max {float(ref.abs().max()):.3e}, worst err / bound "
          f"{float((err / (atol + rtol * ref.abs())).max()):.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance; max abs err {float(err.max()):.3e}"


def _module(C, multiscale):
    from lidar4d_amd.planes_field import Planes4D
    mod = pw.fill_planes(Planes4D(output_dim=C, resolution=pw.RESOLUTION, multiscale_res=multiscale), f"gpu{C}")
    cpu_planes = [[p.detach().clone() for p in coefs] for coefs in mod.planes]
    return mod.to(DEV), cpu_planes


def _out_grads(P, n_out, key):
    return det_uniform((P, n_out), key + ".gs", -1, 1), det_uniform((P, n_out), key + ".gd", -1, 1)


@functools.lru_cache(maxsize=None)
def _sampler_reference(C, multiscale, P):
    """Float64 outputs and gradients of the sampler for one shape, computed once and shared (the tensors are not written to)."""
    _, planes = _module(C, multiscale)
    xt, _ = pw.sample_inputs(P, multiscale, key=f"smp{P}")
    gs, gd = _out_grads(P, len(multiscale) * C, f"smp{P}")
    s, d = pw.planes_fwd(planes, xt, 0)
    grads, dxt = pw.planes_bwd(planes, xt, 0, gs, gd)
    return xt, gs, gd, s, d, grads, dxt


# ---- 1. Planes4D at the new widths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multiscale,P", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("C", [4, 16])
def test_planes4d_vs_float64_reference(C, multiscale, P):
    mod, _ = _module(C, multiscale)
    xt_cpu, gs, gd, ref_s, ref_d, ref_grads, ref_dxt = _sampler_reference(C, multiscale, P)
    xt = xt_cpu.to(DEV).requires_grad_(True)
    fs, fd = mod(xt)
    assert fs.shape == fd.shape == (P, len(multiscale) * C) and fs.dtype == torch.float32
    rel_close(fs, ref_s, 2e-5, 1e-6, "planes static")
    rel_close(fd, ref_d, 2e-5, 1e-6, "planes time")
    rel_close(mod.forward_static(xt), ref_s, 2e-5, 1e-6, "planes static-only")
    rel_close(mod.forward_dynamic(xt), ref_d, 2e-5, 1e-6, "planes time-only")
    ((fs * gs.to(DEV)).sum() + (fd * gd.to(DEV)).sum()).backward()
    rel_close(xt.grad, ref_dxt, 1e-4, 1e-4, "planes d/dxt")
    for s, coefs in enumerate(mod.planes):
        for ci, p in enumerate(coefs):
            rel_close(p.grad, ref_grads[s][ci], 1e-4, 1e-4, f"planes grad {s}.{ci}")


# ---- 2. density_features at all three widths ------------------------------------------------------------------------------------------
def _flow_as(flow, C):
    """The three forms a flow arrives in: dense fp32 [P, 6] (what FlowField returns), fp16 rows of 16 (the fused path's network output),
    fp32 columns 0..5 of rows of 8 -- read in place through the stride argument.  -> (tensor for the call, its fp32 values)"""
    P = flow.shape[0]
    if C == 4:
        return flow.to(DEV), flow
    if C == 8:
        f16 = torch.zeros(P, 16, dtype=torch.float16)
        f16[:, :6] = flow.half()
        f16[:, 6:] = 7.0  # (columns the kernel must not read)
        return f16.to(DEV), f16[:, :6].float()
    wide = torch.full((P, 8), 7.0)
    wide[:, :6] = flow
    return wide.to(DEV)[:, :6], flow


@pytest.mark.parametrize("multiscale,P", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("frame", [0, 25, 50])
@pytest.mark.parametrize("C", [4, 8, 16])
def test_density_features_vs_float64_reference(C, frame, multiscale, P):
    from lidar4d_amd import ops
    mod, planes = _module(C, multiscale)
    xt_cpu, flow_cpu = pw.sample_inputs(P, multiscale, key=f"den{P}.{frame}")
    t_dev = torch.tensor([frame / 50], dtype=torch.float32, device=DEV)
    tinfo = ops.time_setup(t_dev, pw.NUM_FRAMES)
    ti = tinfo.cpu().tolist()
    tinfo_ref = (ti[0], ti[1], ti[2], ti[3] != 0.0, ti[4] != 0.0)
    assert tinfo_ref == pw.time_info(frame / 50, pw.NUM_FRAMES) and tinfo_ref[3:] == (frame < 50, frame > 0)
    xt_cpu[:, 3] = ti[0]
    flow_dev, flow_val = _flow_as(flow_cpu, C)
    assert flow_dev.stride(0) == {4: 6, 8: 16, 16: 8}[C] or P == 1
    n_out = len(multiscale) * C
    gs, gd = _out_grads(P, n_out, f"den{P}")
    ref_s, ref_d = pw.density_fwd(planes, xt_cpu, flow_val, tinfo_ref)
    ref_grads, ref_dflow, ref_dxt = pw.density_bwd(planes, xt_cpu, flow_val, tinfo_ref, gs, gd)

    xt = xt_cpu.to(DEV).requires_grad_(True)
    if C == 8:  # fp16 rows: autograd would hand their gradient back rounded to fp16; the entry point's fp32 dflow is read below
        flow = leaf = flow_dev
    elif flow_dev.is_contiguous():
        flow = leaf = flow_dev.detach().requires_grad_(True)
    else:  # the strided view: the leaf behind it takes the gradient
        leaf = flow_dev._base.detach().requires_grad_(True)
        flow = leaf[:, :6]
    ps, pd = mod.density_features(xt, flow, tinfo)
    assert ps.shape == pd.shape == (P, n_out) and ps.dtype == pd.dtype == torch.float32
    rel_close(ps, ref_s, 2e-5, 1e-6, "plane_s")
    rel_close(pd, ref_d, 2e-5, 1e-6, "plane_d")
    ((ps * gs.to(DEV)).sum() + (pd * gd.to(DEV)).sum()).backward()
    if C == 8:
        dflow, _ = ops.density_planes_bwd(mod.layout, mod._arena(), xt.detach(), flow_dev, tinfo, gs.to(DEV), gd.to(DEV),
                                          torch.zeros(mod.layout.numel, device=DEV), want_dflow=True)
    else:
        dflow = leaf.grad[:, :6]
        if leaf.shape[1] > 6:
            assert not bool(leaf.grad[:, 6:].any())
    rel_close(dflow, ref_dflow, 1e-4, 1e-4, "dflow")
    rel_close(xt.grad, ref_dxt, 1e-4, 1e-4, "d/dxt")
    for s, coefs in enumerate(mod.planes):
        for ci, p in enumerate(coefs):
            rel_close(p.grad, ref_grads[s][ci], 1e-4, 1e-4, f"plane grad {s}.{ci}")
    if frame == 0:
        assert not bool(dflow[:, 3:].any()) and not bool(ref_dflow[:, 3:].any()), "no backward neighbour: its three columns are exactly zero"
        assert bool(dflow[:, :3].any()) or P == 1
    if frame == 50:
        assert not bool(dflow[:, :3].any()) and not bool(ref_dflow[:, :3].any()), "no forward neighbour: its three columns are exactly zero"
        assert bool(dflow[:, 3:].any()) or P == 1


def test_density_features_without_flow_gradient_and_zero_samples():
    """No gradient asked for the flow or the coordinates (a no-grad flow), and P = 0: valid calls."""
    from lidar4d_amd import ops
    mod, planes = _module(4, (1, 2, 4))
    xt_cpu, flow_cpu = pw.sample_inputs(257, (1, 2, 4), key="nograd")
    tinfo = ops.time_setup(torch.tensor([0.5], device=DEV), pw.NUM_FRAMES)
    xt_cpu[:, 3] = 0.5
    ps, pd = mod.density_features(xt_cpu.to(DEV), flow_cpu.to(DEV), tinfo)
    (ps.sum() + pd.sum()).backward()
    ones = torch.ones(257, 12)
    ref_grads, _, _ = pw.density_bwd(planes, xt_cpu, flow_cpu, pw.time_info(0.5, pw.NUM_FRAMES), ones, ones)
    for s, coefs in enumerate(mod.planes):
        for ci, p in enumerate(coefs):
            rel_close(p.grad, ref_grads[s][ci], 1e-4, 1e-4, f"plane grad {s}.{ci}")
    empty = torch.empty(0, 4, device=DEV)
    ps, pd = mod.density_features(empty, torch.empty(0, 6, device=DEV), tinfo)
    assert ps.shape == pd.shape == (0, 12)
    s, d = mod(empty)
    assert s.shape == d.shape == (0, 12)


# ---- 3. old against new at eight channels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multiscale,P", SHAPES, ids=SHAPE_IDS)
def test_width_8_sampler_equals_the_old_kernels(multiscale, P):
    """l4dh_planes_fwd / _bwd against l4d_planes_fwd / _bwd: the forward and d/dxt bit for bit (one kernel, csrc/planes_kernels.h,
    serves both libraries and neither output goes through atomics), the plane gradients within the gradient bound (the atomics'
    order differs from launch to launch)."""
    from lidar4d_amd import ops
    mod, _ = _module(8, multiscale)
    arena = mod._arena()
    xt, _ = pw.sample_inputs(P, multiscale, key=f"w8.{P}")
    xt = xt.to(DEV)
    gs, gd = (g.to(DEV) for g in _out_grads(P, len(multiscale) * 8, f"w8.{P}"))
    for which in (0, 1, 2):
        old = ops.planes_fwd(mod.layout, arena, xt, which, width_lib=False)
        new = ops.planes_fwd(mod.layout, arena, xt, which, width_lib=True)
        for o, n in zip(old, new):
            assert (o is None) == (n is None) and (o is None or torch.equal(o, n)), which
        g_old, g_new = torch.zeros_like(arena), torch.zeros_like(arena)
        ds, dd = (None if which == 2 else gs), (None if which == 1 else gd)
        dxt_old = ops.planes_bwd(mod.layout, arena, xt, which, ds, dd, g_old, True, width_lib=False)
        dxt_new = ops.planes_bwd(mod.layout, arena, xt, which, ds, dd, g_new, True, width_lib=True)
        rel_close(g_new, g_old, 1e-4, 1e-4, f"plane gradients, which = {which}")
        assert torch.equal(dxt_new, dxt_old), which
        assert bool(g_old.any())


@pytest.fixture(scope="module")
def default_model():
    from lidar4d_amd import LiDAR4D
    return fill_model(LiDAR4D(**SMALL_MODEL), seed=7).to(DEV)


@pytest.mark.parametrize("P", [257, 4097])  # (below and above ops.PLANE_ROWS_MIN_POINTS: both forms of the encode's time planes)
@pytest.mark.parametrize("frame", [0, 25, 50])
def test_width_8_density_features_equal_the_fused_encodes_plane_columns(default_model, frame, P):
    """density_features rounded to fp16 against X[:, :2 * n_scales * 8] of the fused field encode on the same inputs: every element
    within one fp16 unit in the last place (floor 2^-24, the subnormal spacing) -- the two evaluate in different orders in fp32 and
    round once."""
    from lidar4d_amd import fused, ops
    model = default_model
    pe = model.planes_encoder
    n_pl = pe.layout.n_scales * 8
    xt = det_uniform((P, 4), f"enc{P}.{frame}", -0.05, 1.05)
    fixed = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [-0.25, 0.5, 1.25, 0.3], [1.25, -0.25, 0.5, 1.0],
                          [1 / 15, 3 / 15, 5 / 15, 0.0], [7 / 31, 9 / 31, 30 / 31, 0.0]])
    xt[:6] = fixed
    flow16 = torch.zeros(P, 16, dtype=torch.float16)
    flow16[:, :6] = det_uniform((P, 6), f"encf{P}", -0.3, 0.3).half()
    tinfo = ops.time_setup(torch.tensor([frame / 50], dtype=torch.float32, device=DEV), model.num_frames)
    xt[:, 3] = float(tinfo[0])
    xt, flow16 = xt.to(DEV), flow16.to(DEV)
    with torch.no_grad():
        X = ops.density_encode_fwd(fused._field_desc(model), xt, flow16, tinfo, model.sigma_net.in_pad)
        ps, pd = pe.density_features(xt, flow16, tinfo)
    got = torch.cat([ps, pd], 1).half().double().cpu()
    want = X[:, :2 * n_pl].double().cpu()
    mag = torch.maximum(got.abs(), want.abs()).clamp_min(2.0 ** -14)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 10)  # >= 2^-24
    err = (got - want).abs()
    print(f"frame {frame} P {P}: {float((err > 0).double().mean()):.4f} of the elements differ, worst {float((err / ulp).max()):.2f} ulp")
    assert bool((err <= ulp).all()), float((err / ulp).max())


# ---- 4. model level ---------------------------------------------------------------------------------------------------------------------
def scale_err(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module", params=[CFG4, CFG16], ids=["C4", "C16"])
def models(request):
    from lidar4d_amd import LiDAR4D
    prev = tcnn_ref.get_precision()
    tcnn_ref.set_precision("tcnn")
    ref = fill_model(fields_ref.LiDAR4D(**request.param), seed=7)
    hip = fill_model(LiDAR4D(**request.param), seed=7).to(DEV)
    assert hip.fused is False
    yield ref, hip
    tcnn_ref.set_precision(prev)


@pytest.mark.parametrize("frame,n_rays,steps,dscale,perturb", [(25, 64, 96, 40.0, True), (0, 16, 768, 8.0, False)])
def test_render_vs_oracle(models, frame, n_rays, steps, dscale, perturb):
    """tests/test_gpu_model.py::test_render_vs_oracle, its assertions as they are, on models of 4 and 16 channels per plane."""
    ref, hip = models
    ref.density_scale = hip.density_scale = dscale
    ro, rd = make_rays(n_rays, 11 + frame)
    noise = det_uniform((n_rays, steps), f"rn{frame}", 0.0, 1.0)
    t = torch.tensor([[frame / 50]])
    ref.zero_grad()
    hip.zero_grad()
    out_ref = ref.render(ro, rd, t, staged=False, num_steps=steps, perturb=perturb, noise=noise)
    out = hip.render(ro.to(DEV), rd.to(DEV), t.to(DEV), staged=False, num_steps=steps, perturb=perturb, noise=noise.to(DEV))
    assert torch.equal(out["z_vals"].cpu(), out_ref["z_vals"]), "sample positions must be bit-exact"
    assert out["depth_lidar"].shape == (1, n_rays) and out["image_lidar"].shape == (1, n_rays, 2)
    assert out["weights"].shape == (n_rays, steps) and out["weights_sum_lidar"].shape == (n_rays,)
    e_depth = scale_err(out["depth_lidar"], out_ref["depth_lidar"])
    e_drop = scale_err(out["image_lidar"][..., 0], out_ref["image_lidar"][..., 0])
    e_int = scale_err(out["image_lidar"][..., 1], out_ref["image_lidar"][..., 1])
    e_w = scale_err(out["weights"], out_ref["weights"])
    print(f"frame {frame}: depth {e_depth:.2e} raydrop {e_drop:.2e} intensity {e_int:.2e} weights {e_w:.2e}")
    assert e_depth < 1e-3 and e_drop < 1e-3 and e_int < 1e-3, (e_depth, e_drop, e_int)
    # weights > 1e-4 index set: identical except where the oracle's weight sits within 1e-3 relative of the threshold
    cnt = int(out["mask_count"])
    got = set(out["mask_idx"][:cnt].tolist())
    want = set(torch.nonzero(out_ref["mask"].reshape(-1)).reshape(-1).tolist())
    wref = out_ref["weights"].reshape(-1)
    diff = got ^ want
    for i in diff:
        assert abs(float(wref[i]) - 1e-4) < 1e-7, (i, float(wref[i]))
    assert len(diff) <= max(2, len(want) // 500), (len(diff), len(want))
    # backward
    gd_ = det_uniform((1, n_rays), "gdep", -1, 1)
    gi_ = det_uniform((1, n_rays, 2), "gimg", -1, 1)
    ((out_ref["depth_lidar"] * gd_).sum() + (out_ref["image_lidar"] * gi_).sum()).backward()
    ((out["depth_lidar"] * gd_.to(DEV)).sum() + (out["image_lidar"] * gi_.to(DEV)).sum()).backward()
    dig_ref, dig = grad_digest(ref), grad_digest(hip)
    worst = 0.0
    for n, v in dig_ref.items():
        scale = max(abs(v[1]), 1e-12)
        err = max(abs(dig[n][0] - v[0]), abs(dig[n][2] - v[2])) / scale
        # |.|-sum compared relatively too
        err = max(err, abs(dig[n][1] - v[1]) / scale)
        worst = max(worst, err)
        assert err < 3e-2, (n, dig[n], v)
    print(f"frame {frame}: worst gradient digest error {worst:.2e}")


def test_staged_render_equals_the_unstaged(models):
    """render(staged=True, max_ray_batch=24): chunks of 24, 24 and 16 rays; every sample is computed on its own, so the results are
    the unstaged ones.  ``graph_staged`` is ignored without the fused pipeline (density() reads the time on the host)."""
    _, hip = models
    hip.density_scale = 40.0
    ro, rd = make_rays(64, 36)
    t = torch.tensor([[0.5]])
    with torch.no_grad():
        out = hip.render(ro.to(DEV), rd.to(DEV), t.to(DEV), staged=False, num_steps=96, perturb=False)
        st = hip.render(ro.to(DEV), rd.to(DEV), t.to(DEV), staged=True, max_ray_batch=24, num_steps=96, perturb=False)
        hip.graph_staged = True
        try:
            st_g = hip.render(ro.to(DEV), rd.to(DEV), t.to(DEV), staged=True, max_ray_batch=16, num_steps=96, perturb=False)
            st_g = hip.render(ro.to(DEV), rd.to(DEV), t.to(DEV), staged=True, max_ray_batch=16, num_steps=96, perturb=False)
        finally:
            hip.graph_staged = False
    assert set(out) == {"depth_lidar", "image_lidar", "weights_sum_lidar", "weights", "z_vals", "mask_idx", "mask_count"}
    assert torch.equal(st["depth_lidar"], out["depth_lidar"]) and torch.equal(st["image_lidar"], out["image_lidar"])
    assert torch.equal(st_g["depth_lidar"], out["depth_lidar"]) and torch.equal(st_g["image_lidar"], out["image_lidar"])
    assert "_chunk_graph" not in hip.__dict__


# ---- 5. one training step -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """One eager Trainer.train_step of the C = 4 model on frame 20 (time 0.4: time slices 2 and 3 of 8), and the same step by
    torch.optim.Adam on an identically filled twin given the same batch and the same sample noise."""
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import SyntheticKitti360
    from lidar4d_amd.trainer import Trainer
    cfg = dict(CFG4, density_scale=20.0)
    data = SyntheticKitti360(DEV, H=16, W=64, num_frames=51, num_rays=64, seed=3)
    model, twin = (fill_model(LiDAR4D(**cfg), seed=11).to(DEV) for _ in range(2))
    # (loss scale 1: the operator-level networks put their own constant 128 on the fp16 adjoints)
    tr = Trainer(model, data, lr=1e-2, iters=100, num_steps=64, flow=False, init_scale=1.0)
    batch = data.batch_for(20)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    torch.manual_seed(5)
    loss = tr.train_step(batch)
    opt = torch.optim.Adam(twin.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    torch.manual_seed(5)
    out = twin.render(batch["rays_o_lidar"], batch["rays_d_lidar"], batch["time"], staged=False, perturb=True, num_steps=64)
    loss_twin = tr.compute_loss(batch, out)
    loss_twin.backward()
    opt.step()
    return tr, model, twin, before, float(loss.detach()), float(loss_twin.detach()), data


def test_train_step_equals_torch_adam(trained):
    tr, model, twin, before, loss, loss_twin, _ = trained
    assert tr.graphs_supported() is False
    with pytest.raises(RuntimeError, match="graphs_supported"):
        tr.train_step_graphed(20)
    assert np.isfinite(loss) and abs(loss - loss_twin) <= 1e-5 * abs(loss_twin), (loss, loss_twin)
    assert float(tr.scaler.state[0]) == 1.0  # (no overflow: the step was taken, the loss scale not halved)
    # the tolerance of tests/test_gpu_optim.py::test_untouched_time_slices_are_left_alone for FlatAdam against torch
    a, b = twin._store.flat, model._store.flat
    close = ((a - b).abs() <= 2e-3 * (1e-2 + a.abs())).float().mean().item()
    assert close > 0.995, close
    moved = 0
    for n, p in model.named_parameters():
        if n.startswith("unet."):
            continue
        if ".hash_t." in n:
            s = int(n.split(".hash_t.")[1].split(".")[0])
            if s in (2, 3):
                assert not torch.equal(p.detach(), before[n]), n
            else:
                assert torch.equal(p.detach(), before[n]), n
        elif not torch.equal(p.detach(), before[n]):
            moved += 1
    # every plane, the static grid, the flow field and the three networks have moved
    assert moved == sum(1 for n, _ in model.named_parameters() if not n.startswith("unet.") and ".hash_t." not in n and before[n].numel())
    gates = model._store.gates
    assert gates[:8].ne(0).tolist() == [False, False, True, True, False, False, False, False]


def test_evaluate_refine_data_and_checkpoint(trained, tmp_path):
    """Trainer.evaluate, collect_refine_data and a checkpoint round trip with a model that has no fused pipeline."""
    from lidar4d_amd import LiDAR4D
    tr, model, _, _, _, _, data = trained
    res = tr.evaluate(frames=[20], refine=False, max_ray_batch=300)
    assert np.isfinite(float(res["loss"]))
    inp, gt = tr.collect_refine_data(frames=[20], max_ray_batch=300)
    assert inp.shape == (1, 3, 16, 64) and gt.shape == (1, 1, 16, 64) and bool(torch.isfinite(inp).all())
    path = tr.save(str(tmp_path / "c4.pth"), epoch=1)
    other = LiDAR4D(**dict(CFG4, density_scale=20.0)).to(DEV)
    from lidar4d_amd.checkpoint import load_checkpoint
    info = load_checkpoint(path, other)
    assert not info["missing_keys"] and not info["unexpected_keys"]
    fr = data.frame(20)
    with torch.no_grad():
        a = model.render(fr["rays_o_lidar"][:, :50], fr["rays_d_lidar"][:, :50], fr["time"], staged=False, num_steps=64, perturb=False)
        b = other.render(fr["rays_o_lidar"][:, :50], fr["rays_d_lidar"][:, :50], fr["time"], staged=False, num_steps=64, perturb=False)
    assert torch.equal(a["depth_lidar"], b["depth_lidar"]) and torch.equal(a["image_lidar"], b["image_lidar"])
