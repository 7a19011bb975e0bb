"""The fused patch depth-gradient loss (csrc/patchgrad.hip, lidar4d_amd.trainer.patch_depth_grad_loss) on the device (``-m gpu``,
MI355X): against the reference's own train_step (tests/golden/train_step_losses.npz), against the torch restatement
``depth_grad_loss`` it replaces in the step, with fp16 ground truth, bit-for-bit against itself; the patch batch on the fused
draw; and inside a Trainer: eager, as a captured step, and alternating with single-pixel epochs.

Bounds.  Against the fixture: the rule of train_golden.check at rtol = 1e-4, what the other fused nodes use against the same file.
Against ``depth_grad_loss`` on the device: 2e-5 relative on the value and 2e-5 of the largest magnitude on the gradient, the
project's figure for a fused node against its restatement; every element-wise value is formed by the same fp32
operations, so the two differ by the order of the sums (fp64 here, fp32 trees in torch) and, for the cosine criterion, by the
rounding of the per-patch norms.  The cases and why they are these: tests/patchgrad_cases.py."""
import numpy as np
import pytest
import torch

import patchgrad_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 2e-5
UPSTREAM = (1.0, 512.0)
TERMS = {
    "main": dict(),
    "all4": dict(grad_norm_smooth=True, spatial_smooth=True, tv_loss=True),
    "smooth_only": dict(grad_loss=False, grad_norm_smooth=True, spatial_smooth=True, tv_loss=True),
}
_cache = {}


def _case(name, sobel=False, flat=True, half=False):
    """Sobel cases at a power-of-two scale (exact stencil sums in any order), the others at the KITTI-360 scale."""
    key = (name, sobel, flat, half)
    if key not in _cache:
        c = pc.make(name, scale=pc.SCALE_POW2 if sobel else pc.KITTI360_SCALE, flat=flat, half=half)
        _cache[key] = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    return _cache[key]


def _reference(key, c, upstream, kw):
    from lidar4d_amd.trainer import depth_grad_loss
    key = ("ref", key, upstream, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = pc.run(depth_grad_loss, c, upstream=upstream, **kw)
    return _cache[key]


def _compare(label, c, ckey, kw):
    from lidar4d_amd.trainer import patch_depth_grad_loss
    for upstream in UPSTREAM:
        want, g_want = _reference(ckey, c, upstream, kw)
        got, g_got = pc.run(patch_depth_grad_loss, c, upstream=upstream, **kw)
        g_scale = float(g_want.abs().max())
        err_l = abs(float(got) - float(want))
        err_g = float((g_got - g_want).abs().max())
        print(f"{label} x{upstream:g}: loss {float(got):.9g} (torch {float(want):.9g}, rel {err_l / max(abs(float(want)), 1e-30):.2e}), "
              f"gradient err / max = {err_g / max(g_scale, 1e-30):.2e} (max {g_scale:.3g})")
        assert bool(torch.isfinite(g_want).all()) and bool(torch.isfinite(g_got).all())
        assert err_l <= RTOL * abs(float(want))
        assert err_g <= RTOL * g_scale
        assert g_got.shape == c["pred"].shape and g_got.dtype == c["pred"].dtype == torch.float32
    return g_got


# ---- 1. the reference's own train_step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["patch_sobel_cos_all", "patch_mse_tv", "everything", "patch_l1"])
def test_fused_term_vs_reference_train_step(tag, monkeypatch):
    """tests/golden/train_step_losses.npz (the loss block of the reference's Trainer.train_step): the total loss with the patch
    terms from the fused node and every other term from the torch functions, and every gradient.  ``patch_l1``'s term is
    identically zero in the fixture (its ground truth has no smooth neighbour pairs): there the case shows only that the node
    returns an exact 0 and a zero gradient."""
    from lidar4d_amd import trainer as T
    from tests import train_golden
    c = train_golden.load(tag)
    assert train_golden.opt_of(c)["patch_size_lidar"] != 1
    entered = []

    def fused(*a, **kw):
        entered.append(kw.get("kind"))
        loss = T.patch_depth_grad_loss(*a, **kw)
        if tag == "patch_l1":
            assert float(loss) == 0.0
        return loss

    monkeypatch.setattr(T, "depth_grad_loss", fused)
    loss, leaves = train_golden.evaluate(c, device=DEV)
    assert entered == [train_golden.opt_of(c)["depth_grad_loss"]]
    train_golden.check(c, loss, leaves, rtol=1e-4)


# ---- 2. the torch restatement on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("sobel", [False, True])
@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("name", ["6x2x8", "8x3x3"])
def test_fused_term_vs_depth_grad_loss(name, kind, sobel, terms):
    flat = kind != "cos"
    c = _case(name, sobel=sobel, flat=flat)
    kw = dict(kind=kind, sobel_grad=sobel, **TERMS[terms])
    g = _compare(f"{name} {kind} sobel={sobel} {terms}", c, (name, sobel, flat), kw)
    if name == "6x2x8" and terms == "main":
        assert float(g.reshape(6, 2, 8)[pc.ALL_DROPPED].abs().max()) == 0.0  # the all-dropped patch: exactly no gradient


@pytest.mark.parametrize("config", ["default", "cos_sobel"])
@pytest.mark.parametrize("name", ["1x2x2", "4x4x8", "3x8x16", "300x2x8", "1x32x32"])
def test_fused_term_vs_depth_grad_loss_other_shapes(name, config):
    sobel = config == "cos_sobel"
    kw = dict(kind="cos", sobel_grad=True) if sobel else dict()
    _compare(f"{name} {config}", _case(name, sobel=sobel), (name, sobel, True), kw)


@pytest.mark.parametrize("config", ["huber_all4", "cos", "huber_all4_sobel", "cos_sobel"])
@pytest.mark.parametrize("name", list(pc.STRIDE_CASES))
def test_fused_term_past_its_grid(name, config):
    """pc.STRIDE_CASES: more groups than PG_MAX_BLOCKS workgroups, for patches of at most a wavefront (4101 x 8 x 8: 1026 groups of
    four) and for large ones (1030 x 5 x 13: a group each), so that a workgroup sweeps a second group over the LDS images of its
    first; 262,464 elements, past the 1024 x 256 that pg_scale_kernel covers in one turn; and 35-pixel patches, one to a
    wavefront with idle lanes.  The same comparison and bound as every other shape."""
    sobel = config.endswith("_sobel")
    kw = dict(kind="cos") if config.startswith("cos") else dict(kind="huber", **TERMS["all4"])
    n, px, py = pc.shape_of(name)
    assert (n > 1024 * (1 if px * py > 64 else 4 * (64 // (px * py)))) == (name != "9x5x7")
    _compare(f"{name} {config}", _case(name, sobel=sobel), (name, sobel, True), dict(kw, sobel_grad=sobel))


# ---- 3. fp16 ground truth -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", ["main", "all4"])
@pytest.mark.parametrize("kind", ["l1", "mse"])  # (the restatement's huber_loss refuses a half target)
@pytest.mark.parametrize("name", ["6x2x8", "8x3x3"])
def test_fp16_ground_truth(name, kind, terms):
    c = _case(name, half=True)
    assert c["gt"].dtype == torch.float16 and c["hit"].dtype == torch.float16
    _compare(f"{name} fp16 {kind} {terms}", c, (name, "half"), dict(kind=kind, **TERMS[terms]))


def test_fp16_ground_truth_with_sobel_is_refused():
    from lidar4d_amd.trainer import patch_depth_grad_loss
    c = _case("6x2x8", half=True)
    with pytest.raises(ValueError, match="fp16"):
        patch_depth_grad_loss(c["pred"], c["gt"], c["hit"], c["patch_size"], c["scale"], sobel_grad=True)


# ---- 4. same bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("300x2x8", dict(kind="huber", **TERMS["all4"])), ("3x8x16", dict(kind="cos", sobel_grad=True)),
                                     ("8x3x3", dict(kind="cos")), ("4101x8x8", dict(kind="huber", **TERMS["all4"]))])
def test_same_input_same_bits(name, kw):
    from lidar4d_amd.trainer import patch_depth_grad_loss
    c = _case(name, sobel=bool(kw.get("sobel_grad")))
    a, ga = pc.run(patch_depth_grad_loss, c, upstream=512.0, **kw)
    torch.empty(1 << 20, device=DEV).fill_(float("nan"))  # (the workspace of the second call is not the first call's, nor clean)
    b, gb = pc.run(patch_depth_grad_loss, c, upstream=512.0, **kw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))


# ---- 5. the patch batch on the fused draw -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch,rays", [([2, 8], 144), (3, 144), ([2, 8], 256)], ids=["patch0", "3", "patch0-256"])
def test_patch_batch_fused_vs_torch(patch, rays):
    """SyntheticKitti360.batch_for on a patch batch: the draw with the patches expanded in the kernel (data.draw_ray_batch) against
    the same dataset's torch route for the same seed.  144 rays: 9 patches of 2 x 8, 16 of 3 x 3; 256: a full workgroup of 2 x 8."""
    from lidar4d_amd.data import SyntheticKitti360
    out = {}
    for fused in (True, False):
        data = SyntheticKitti360(DEV, H=16, W=64, num_frames=3, num_rays=rays, seed=11)
        data.fused_batch, data.patch_size_lidar = fused, patch
        out[fused] = (data.batch_for(1), data.batch_for(2), data.gen.get_state())
    for k in (0, 1):
        a, b = out[True][k], out[False][k]
        assert a["images_lidar"].shape == (1, rays, 3) and torch.equal(a["images_lidar"], b["images_lidar"])
        assert torch.equal(a["rays_o_lidar"], b["rays_o_lidar"])
        assert float((a["rays_d_lidar"] - b["rays_d_lidar"]).abs().max()) <= 2e-7
    assert torch.equal(out[True][2], out[False][2])  # both generators in the same state
    assert not torch.equal(out[True][0]["images_lidar"], out[True][1]["images_lidar"])


# ---- 6. inside the Trainer ------------------------------------------------------------------------------------------------------------
def _small_trainer(patch=(2, 8), **kw):
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.trainer import Trainer
    from oracle.detparams import fill_model
    from oracle.make_golden import SMALL_MODEL
    cfg = dict(SMALL_MODEL, num_frames=5, near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE, density_scale=20.0)
    data = SyntheticKitti360(DEV, H=16, W=64, num_frames=5, num_rays=128)
    if patch is not None:
        data.patch_size_lidar = list(patch)
    m = fill_model(LiDAR4D(**cfg), seed=3, flow_out_amp=0.002).to(DEV)
    return m, data, Trainer(m, data, num_steps=64, chamfer=False, flow=False, init_scale=1.0, **kw)


def test_trainer_compute_loss_fused_vs_torch():
    """Trainer.compute_loss on the same render outputs with the fused node and with ``depth_grad_loss``: value, and the gradient
    that reaches the render's ``depth_lidar``.  On the CPU the synthetic frames at 16 x 64 give 62 - 75 masked-in pairs of 112 and
    a term of 0.6 - 0.9."""
    m, data, tr = _small_trainer(iters=10)
    assert tr.fused_patch and tr.graphs_supported()
    batch = data.batch_for(2)
    out = m.render(batch["rays_o_lidar"], batch["rays_d_lidar"], batch["time"], staged=False, perturb=False, num_steps=64,
                   time_host=batch.get("time_host"))
    res = {}
    for fused in (True, False):
        tr.fused_patch = fused
        loss = tr.compute_loss(batch, out)
        (g,) = torch.autograd.grad(loss, out["depth_lidar"], retain_graph=True)
        res[fused] = (float(loss), g)
    assert not tr.graphs_supported()  # the torch route
    data.patch_size_lidar = 1
    plain = float(tr.compute_loss(batch, out))
    (lf, gf), (lt, gt_) = res[True], res[False]
    print(f"compute_loss: fused {lf:.8g}, torch {lt:.8g}; without the term {plain:.8g}")
    assert lt - plain > 1e-3 * lt, "the patch term is too small a part of this loss to be checked by it"
    assert abs(lf - lt) <= RTOL * abs(lt)
    assert float(gt_.abs().max()) > 0 and float((gf - gt_).abs().max()) <= RTOL * float(gt_.abs().max())


# ---- 7. a captured patch step -----------------------------------------------------------------------------------------------------------
def test_captured_patch_step_equals_eager_step(monkeypatch):
    """A [2, 8] step can be captured, and a REPLAY reproduces the eager step from the same state and batch (the scheme and the
    bounds of test_graph_replay_equals_eager_step: static batch, no sample jitter, snapshot / restore; gradients within 1e-3 of
    each tensor's largest value -- the order of the dW atomics -- and at most 1e-4 of the parameters off by more than 1e-4)."""
    from lidar4d_amd.params import bump_epoch
    m, data, tr = _small_trainer(iters=16, graph_batch_inside=False)
    assert tr.graphs_supported()
    st, opt = m._store, tr.opt
    batch = {k: (v.contiguous().clone() if torch.is_tensor(v) else v) for k, v in data.batch_for(2).items()}
    assert batch["rays_d_lidar"].shape[1] == 128
    monkeypatch.setattr(data, "batch_for", lambda frame: batch)
    render = m.render
    monkeypatch.setattr(m, "render", lambda *a, **kw: render(*a, **{**kw, "perturb": False}))
    for _ in range(3):
        tr.train_step(batch)
    opt.device_schedule()
    snap = {"flat": st.flat.detach().clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(), "steps": opt.steps.clone(),
            "scaler": tr.scaler.state.clone(), "sched": opt.sched.clone(), "count": opt.step_count}

    def restore():
        with torch.no_grad():
            st.flat.copy_(snap["flat"]), opt.exp_avg.copy_(snap["m"]), opt.exp_avg_sq.copy_(snap["v"]), opt.steps.copy_(snap["steps"])
            tr.scaler.state.copy_(snap["scaler"]), opt.sched.copy_(snap["sched"])
        opt.step_count = snap["count"]
        bump_epoch()
        st.refresh16()

    restore()
    l_e = float(tr.train_step(batch))
    g_e, p_e = st.flat_grad.detach().clone(), st.flat.detach().clone()
    assert np.isfinite(l_e) and bool(torch.isfinite(g_e).all()) and not torch.equal(p_e, snap["flat"])
    restore()
    tr.train_step_graphed(2)  # eager warm-up + capture
    assert list(tr._step_graphs["graphs"]) == [(2, (2, 8))]
    for k in range(3):
        restore()
        loss = float(tr.train_step_graphed(2))
        print(f"replay {k}: loss {loss:.8g}, eager {l_e:.8g}")
        assert abs(loss - l_e) <= RTOL * abs(l_e), f"replay {k}: loss {loss} against the eager step's {l_e}"
        for name, p, off, n, gi in st.entries:
            if not n:
                continue
            a, b = st.flat_grad[off:off + n], g_e[off:off + n]
            assert bool(torch.isfinite(a).all()), f"replay {k}: non-finite gradient in {name}"
            d = float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)
            assert d < 1e-3, f"replay {k}: gradient of {name} differs from the eager step's by {d:.2e} of its largest value"
        off_frac = float(((st.flat - p_e).abs() > 1e-4).float().mean())
        assert off_frac < 1e-4, f"replay {k}: {off_frac:.2e} of the parameters differ from the eager step's"


# ---- 8. patch epochs alternate, captured ------------------------------------------------------------------------------------------------
def test_patch_epochs_alternate_with_capture():
    m, data, tr = _small_trainer(patch=None, iters=100, change_patch_size_lidar=[2, 8], epoch_steps=2, graph_batch_inside=True)
    assert tr.graphs_supported()
    losses, sizes = [], []
    for _ in range(8):
        losses.append(float(tr.train_step_graphed(frame=1)))
        sizes.append(data.patch_size_lidar)
    assert sizes == [1, 1, [2, 8], [2, 8], 1, 1, [2, 8], [2, 8]]
    assert sorted(tr._step_graphs["graphs"], key=str) == sorted([(1, 1), (1, (2, 8))], key=str)
    assert all(np.isfinite(losses)), losses
    replays = [losses[3], losses[6], losses[7]]  # (step 2 is the capture call: an eager step)
    print("patch-graph replays:", replays)
    assert len({round(v, 6) for v in replays}) > 1, "the replays of the patch graph see the same batch: the draw is not inside the graph"
