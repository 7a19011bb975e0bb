"""CPU tests that pin the references of tests/loss_ref.py -- what tests/test_gpu_loss_edges.py holds csrc/losses.hip and
csrc/stepglue.hip to -- against the torch restatements ``urf_loss`` and ``lidar_loss`` in float64, and that measure how far a
float32 evaluation sits from them: the yardsticks for the device bounds.  Every case builder is checked to have made the situation
it names.  (``pytest -s`` shows the measured figures.)"""
import numpy as np
import pytest
import torch

import loss_ref as L
import realdata_cases as rc

F16, F32, F64 = np.float16, np.float32, np.float64


# ---- line-of-sight loss -------------------------------------------------------------------------------------------------------------
def _urf(w, z, d, step, dtype, upstream=1.0):
    from lidar4d_amd.trainer import urf_loss
    cast = (lambda t: t.to(dtype)) if dtype is not None else (lambda t: t)
    leaf = cast(w).clone().requires_grad_(True)
    loss = urf_loss({"weights": leaf, "z_vals": cast(z)}, (cast(d) if d.dtype != torch.float16 else d).reshape(1, -1), step, L.ITERS)
    (loss * upstream).backward()
    return float(loss), leaf.grad.numpy()


@pytest.mark.parametrize("name", list(L.LOS_CASES))
def test_los_case_builders_make_the_cases_they_name(name):
    L.assert_los_case(name)


@pytest.mark.parametrize("name", list(L.LOS_CASES_OFF_BOUNDS))
def test_los_ref64_vs_urf_loss_in_float64(name):
    """los_ref64 against ``urf_loss`` and its autograd on float64 tensors, loss and gradient within 1e-12 relative.  The float64
    evaluation forms its bounds in float64, so the cases are the ones without a sample on a bound (every sample at least 1e-5 from
    every bound: assert_los_case shows the two evaluations then take the same near / empty sets), and it divides by the float64
    2 sigma^2, which the reference is told to do as well (``exact_two_var``); the default float32 divisor moves the result by
    less than 3e-7, asserted here too."""
    w, z, d = L.los_case(name, off_bounds=True)
    for step in L.STEPS:
        for upstream in (1.0, 512.0):
            want, g_want = _urf(w, z, d, step, torch.float64, upstream)
            got, g_got = L.los_ref64(w.numpy(), z.numpy(), d.numpy(), step, L.ITERS, upstream, exact_two_var=True)
            err_l, err_g = abs(got - want) / want, float(np.abs(g_got - g_want).max() / np.abs(g_want).max())
            assert want > 0 and err_l <= 1e-12 and err_g <= 1e-12, (name, step, err_l, err_g)
        kern, g_kern = L.los_ref64(w.numpy(), z.numpy(), d.numpy(), step, L.ITERS, 512.0)
        assert abs(kern - got) <= 3e-7 * got and float(np.abs(g_kern - g_got).max()) <= 3e-7 * float(np.abs(g_got).max())


@pytest.mark.parametrize("name", [n for n in L.LOS_CASES if n != "4x8_all_dropped"])
def test_los_ref64_vs_urf_loss_in_float32(name):
    """The float32 restatement on the CPU against los_ref64, on-bound samples and the fp16 depths included (float32 torch takes the
    decisions the way the kernel does): the deviation is printed and is at most 5e-7 -- the yardstick for the device bound of
    1e-6."""
    w, z, d = L.los_case(name)
    for step in L.STEPS:
        want, g_want = L.los_reference(name, step)
        got, g_got = _urf(w, z, d, step, None)
        err_l, err_g = abs(got - want) / want, float(np.abs(g_got - g_want).max() / np.abs(g_want).max())
        print(f"{name} step {step}: fp32 urf_loss against los_ref64: loss {err_l:.2e}, gradient / max {err_g:.2e}")
        assert err_l <= 5e-7 and err_g <= 5e-7


def test_no_ray_with_a_return_gives_the_ieee_pattern():
    """n_hit == 0.  The loss: ``urf_loss`` in float64 and in float32 gives what los_ref64 gives -- +inf, the sum of two positive
    sums divided by 0.  The gradient: los_ref64 is 0.2 * term / n_hit, so +-inf by the term's sign and NaN where the term is 0 (a
    sample on a bound, a weight of 0), which is what l4dl_los_bwd's ``coef * term`` gives; torch's autograd multiplies the inf of
    1 / n_hit with the masks' zeros and returns NaN for EVERY sample, so the gradient pattern of the restatement is not the
    reference's, and the device test holds the kernel to the reference."""
    w, z, d = L.los_case("4x8_all_dropped")
    for step in L.STEPS:
        want, g_want = L.los_reference("4x8_all_dropped", step)
        n_nan = 2 if step == 0 else 1  # the weight of 0, and at step 0 the sample on that step's bound
        assert want == np.inf and int(np.isnan(g_want).sum()) == n_nan and int(np.isinf(g_want).sum()) == 32 - n_nan
        assert int(np.isneginf(g_want).sum()) == 3  # the near samples: w < bell
        for dtype in (torch.float64, torch.float32):
            got, g_got = _urf(w, z, d, step, dtype)
            assert L.same_pattern(got, want)
            assert bool(np.isnan(g_got).all())


def test_same_pattern_tells_the_patterns_apart():
    a = np.array([np.nan, np.inf, -np.inf, 1.0])
    assert L.same_pattern(a, a.copy()) and L.same_pattern(np.array([np.nan, np.inf, -np.inf, -7.0]), a)
    for i, v in ((0, 1.0), (1, -np.inf), (2, np.nan), (3, np.inf)):
        b = a.copy()
        b[i] = v
        assert not L.same_pattern(b, a)


# ---- primary losses -----------------------------------------------------------------------------------------------------------------
PIN_SCALE = 5 * 2.0 ** -9  # 0.2 * PIN_SCALE is DELTA exactly, in float64 and in float32: lidar_loss's Huber delta is the kernel's


def _plain_criterion(kind, scale=1.0):
    """trainer.criterion without its casts to float32 (the autocast policy): the target is widened to the prediction's type."""
    fn = {"l1": lambda a, b: (a - b).abs(), "mse": lambda a, b: (a - b) ** 2,
          "bce": lambda a, b: torch.nn.functional.binary_cross_entropy_with_logits(a, b, reduction="none"),
          "huber": lambda a, b: torch.nn.functional.huber_loss(a, b, reduction="none", delta=0.2 * scale)}[kind]
    return lambda a, b: fn(a, b.to(a.dtype))


def _lidar_loss64(monkeypatch, depth, image, gt, kinds, alphas, smooth):
    from lidar4d_amd import trainer as T
    monkeypatch.setattr(T, "criterion", _plain_criterion)
    a_d, a_r, a_i, s32 = (float(F32(v)) for v in (*alphas, smooth))
    d64 = torch.from_numpy(depth).double()[None].requires_grad_(True)
    i64 = torch.from_numpy(image).double()[None].requires_grad_(True)
    t = torch.from_numpy(gt)[None]
    loss = T.lidar_loss({"depth_lidar": d64, "image_lidar": i64}, t if gt.dtype == F16 else t.double(), a_d, a_r, a_i, s32,
                        depth_loss=kinds[0], raydrop_loss=kinds[1], intensity_loss=kinds[2], scale=PIN_SCALE)
    loss.backward()
    return float(loss), d64.grad[0].numpy(), i64.grad[0].numpy()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_primary_losses_ref64_vs_lidar_loss_in_float64(half, monkeypatch):
    """primary_losses_ref64 against ``lidar_loss`` and its autograd with float64 predictions, all 64 criterion triples, loss and
    both gradients within 1e-12 of each output's largest magnitude (``criterion``'s casts to float32 are taken out; the
    expressions stay).  fp32 ground truth is widened to float64; fp16 ground truth goes in as the half tensor, so that torch takes
    the masked products and the clamp in half as the step does.  One constant is handed over: for fp32 ground truth the float64
    evaluation's upper smoothing target is the float64 1 - smooth, up to 2^-25 from step_gt's float32 one."""
    assert 0.2 * PIN_SCALE == L.DELTA == float(F32(L.DELTA))
    for smooth, alphas in L.SETTINGS:
        s32 = float(F32(smooth))
        upper = None if half else 1.0 - s32
        assert abs(float(L.upper_target(smooth, False)) - (1.0 - s32)) < 2.0 ** -25
        if half:  # torch's clamp of a half tensor lands on the bounds step_gt<true> uses
            got = torch.tensor([0.0, 1.0]).half().clamp(s32, 1 - s32).float().numpy()
            assert np.array_equal(got, [F32(F16(F32(smooth))), L.upper_target(smooth, True)])
        for n in (257,):
            depth, image, gt, rays_d, _ = L.primary_inputs(n, half, 5, smooth)
            for kinds in L.TRIPLES:
                ref = L.primary_losses_ref64(depth, image, gt, rays_d, kinds, alphas, smooth, L.DELTA, PIN_SCALE, upper=upper)
                loss, g_depth, g_image = _lidar_loss64(monkeypatch, depth, image, gt, kinds, alphas, smooth)
                for name, want in (("loss", np.array([loss])), ("g_depth", g_depth), ("g_image", g_image)):
                    top = float(np.abs(want).max())
                    assert np.isfinite(want).all() and top > 0
                    assert float(np.abs(ref[name] - want).max()) <= 1e-12 * top, (kinds, smooth, name)
                assert np.array_equal(ref["gt32"], gt.astype(F32))


def test_planted_block_holds_what_it_says():
    for half in (False, True):
        for smooth, _ in L.SETTINGS:
            depth, image, gt, rays_d, S = L.primary_inputs(257, half, 3, smooth)
            m, gt_i, gt_d, gs, raw = L._gt_terms(gt, F32(smooth))
            delta = F32(L.DELTA)
            assert gt.dtype == (F16 if half else F32) and not m[L.DROPPED_ROWS].any() and m[L.EXACT_ROW] == 1
            e_d, e_i, e_r = depth * m - gt_d, image[:, 1] * m - gt_i, image[:, 0] - gs  # float32, as the kernel subtracts
            assert e_d[L.EXACT_ROW] == 0 and e_i[L.EXACT_ROW] == 0 and e_r[L.EXACT_ROW] == 0
            step = F32(L.LATTICE)
            want = np.array([delta, -delta, delta + step, -(delta + step), delta - step, -(delta - step)], F32)
            assert np.array_equal(e_d[L.HUBER_ROWS], want) and np.array_equal(e_i[L.HUBER_ROWS], want)
            if smooth in (0.0, 0.5):
                assert np.array_equal(e_r[L.HUBER_ROWS], want)
            assert sorted(set(np.abs(depth[L.LOGIT_ROWS]).tolist())) == sorted(set(abs(float(F32(v))) for v in L.LOGITS))
            with np.errstate(over="ignore", under="ignore"):
                assert np.isinf(np.exp(-F32(-89.0))) and np.isfinite(np.exp(-F32(-88.0)))
                assert np.exp(-F32(104.0)) == 0 and np.exp(-F32(88.0)) > 0
            lo, hi = gs[m == 0], gs[m == 1]
            assert len(set(lo.tolist())) == 1 and len(set(hi.tolist())) == 1 and (smooth != 0.5 or lo[0] == hi[0] == 0.5)
    for n in L.PRIMARY_N:
        rows = {float(L.primary_inputs(1, False, s, 0.2)[0][0]) for s in range(L.N_PLANTED)}
        assert len(L.primary_inputs(n, True, n, 0.2)[0]) == n and len(rows) > 20


def test_emulation_of_the_default_criteria_has_the_bits_of_the_existing_reference():
    for n in L.PRIMARY_N + (1000,):
        for smooth, alphas in L.SETTINGS:
            depth, image, gt, rays_d, S = L.primary_inputs(n, False, n, smooth)
            new = L.primary_losses_emul(depth, image, gt, rays_d, ("l1", "mse", "mse"), alphas, smooth, 0.2 * S, S)
            old = rc.primary_losses_ref(depth, image, gt, rays_d, *alphas, smooth, S)
            for name in old:
                assert new[name].tobytes() == old[name].tobytes(), (n, smooth, name)


def test_emulation_against_float64():
    """primary_losses_emul against primary_losses_ref64 on the inputs of the device test: the largest deviation per output in
    units of 2^-24 of that output's largest magnitude, printed per criterion family.  Without BCE the figures only describe
    float32 arithmetic (the device test demands the emulation's bits there).  With BCE they are the measured input to the
    device bound, four times L.BCE_DEVIATION: the measurement may not exceed what that table states."""
    worst = {fam: dict(loss=0.0, g_depth=0.0, g_image=0.0, pts=0.0) for fam in ("bce-free", "with bce")}
    for half in (False, True):
        for n in L.PRIMARY_N:
            for smooth, alphas in L.SETTINGS:
                depth, image, gt, rays_d, S = L.primary_inputs(n, half, n, smooth)
                for kinds in L.TRIPLES:
                    args = (depth, image, gt, rays_d, kinds, alphas, smooth, L.DELTA, S)
                    emul, ref = L.primary_losses_emul(*args), L.primary_losses_ref64(*args)
                    fam = worst["with bce" if "bce" in kinds else "bce-free"]
                    for name in fam:
                        assert np.isfinite(emul[name]).all() and np.isfinite(ref[name]).all()
                        fam[name] = max(fam[name], L.deviation_units(emul[name], ref[name]))
                    assert np.array_equal(emul["gt32"], ref["gt32"])
    for fam, w in worst.items():
        print(f"primary_losses_emul against primary_losses_ref64, {fam}: " + ", ".join(f"{k} {v:.2f}" for k, v in w.items())
              + "  (x 2^-24 of the output's largest magnitude)")
    for name, stated in L.BCE_DEVIATION.items():
        assert worst["with bce"][name] <= stated and stated <= 1.5 * worst["with bce"][name] + 0.5, (name, worst["with bce"][name], stated)
    assert worst["with bce"]["pts"] <= 2.0 and worst["bce-free"]["pts"] <= 2.0  # a product and a quotient


def test_saturated_logits_in_the_references():
    """At |logit| >= 104 the sigmoid in front of a BCE ray-drop term is exactly 0 or 1 in float32 and the chain factor exactly 0,
    so the ray-drop gradient is a zero (from +17 up the float32 sigmoid is 1 already; at -20 it is 2e-9 and the gradient is not
    0); everything stays finite at every planted logit."""
    depth, image, gt, rays_d, S = L.primary_inputs(257, False, 1, 0.2)
    out = L.primary_losses_emul(depth, image, gt, rays_d, ("bce", "bce", "bce"), (1.0, 0.01, 0.1), 0.2, L.DELTA, S)
    assert all(np.isfinite(v).all() for v in out.values())
    sat = np.flatnonzero(np.abs(image[:, 0]) >= 104.0)
    assert sat.size == 8 and (out["g_image"][sat, 0] == 0).all() and (out["g_image"][(image[:, 0] >= -20.0) & (image[:, 0] < 16.0), 0] != 0).all()


# ---- ray batch ----------------------------------------------------------------------------------------------------------------------
def test_ray_batch_ref64_vs_get_lidar_rays():
    """ray_batch_ref64 inside the frame against the whole frame's rays of data.get_lidar_rays (float32: 2e-7 + its own rounding),
    and its out-of-frame conventions."""
    from lidar4d_amd.data import get_lidar_rays
    H, W, fov = 8, 32, (2.0, 26.9)
    g = torch.Generator().manual_seed(0)
    pose = torch.eye(4)
    pose[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    pose[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    image = torch.rand(H, W, 3, generator=g).numpy()
    top, left = np.array([0, H - 2, 3]), np.array([W - 3, 0, 17])
    inds, rays_o, rays_d, gt = L.ray_batch_ref64(top, left, 2, 8, pose.numpy(), fov, H, W, image)
    rays = get_lidar_rays(pose[None], torch.tensor(fov), H, W, -1)
    assert inds.min() >= 0 and inds.max() < H * W and (inds % W).max() == W - 1 and (inds % W).min() == 0
    assert np.array_equal(rays_o, rays["rays_o"][0, inds].numpy()) and np.array_equal(gt, image.reshape(-1, 3)[inds])
    assert float(np.abs(rays_d - rays["rays_d"][0, inds].double().numpy()).max()) <= 4e-7
    inds, _, rays_d, gt = L.ray_batch_ref64(np.array([-3, H - 1]), np.array([-W - 2, 2 * W + 3]), 3, 8, pose.numpy(), fov, H, W,
                                           image.astype(F16))
    rows = np.repeat(np.array([-3, -2, -1, H - 1, H, H + 1]), 8)
    cols = np.concatenate([(np.arange(8) + s) % W for s in (W - 2, W - 2, W - 2, 3, 3, 3)])
    assert np.array_equal(inds, rows * W + cols) and gt.dtype == F16
    assert not gt[rows != H - 1].any() and np.array_equal(gt[rows == H - 1], image.astype(F16)[H - 1, cols[rows == H - 1]])
    assert np.isfinite(rays_d).all() and np.allclose(np.linalg.norm(rays_d, axis=1), 1.0, atol=1e-6)
