"""The evaluation meters on the device (``-m gpu``, MI355X): l4de_image_errors (csrc/evalmeter.hip) against the float64
restatement of tests/meters_ref.py, DepthMeter / IntensityMeter on top of it, and Trainer.evaluate.

Bounds.  Device and restatement clamp and subtract in fp32 identically and work in fp64 from there on, so they differ by the
order of fp64 sums only: RMSE within 1e-10 relative (worst case N * 2^-53 = 8e-12 at 67,980 pixels; max(1e-10, 4 N 2^-53) for the
two sizes past the kernels' bounded grids, see _check_row), SSIM and PSNR within 1e-9
absolute (two fp64 summation orders of the restatement differ by 1e-15).  The median is a selection, not a sum: bit-equal to
np.median of the float32 |d|.  The mean over a meter's updates is one more fp64 sum of a few values: 4 ulp."""
import functools

import numpy as np
import pytest
import torch

import meters_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS64 = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pred, gt, hi, errors_f64) of a shared case: computed once, never written to."""
    H, W, hi = ref.CASES[name][:3]
    pred, gt = ref.make_pair(*ref.CASES[name])
    want = ref.errors_f64(pred, gt, ref.LO, hi)
    for a in (pred, gt, want):
        a.setflags(write=False)
    return pred, gt, hi, want


def _device_errors(pred, gt, lo, hi):
    from lidar4d_amd.metrics import image_errors
    out = image_errors(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), lo, hi)
    assert out.dtype == torch.float64 and out.shape == (4,) and out.is_cuda
    return out.cpu().numpy()


def _check_row(got, want, tag="", medae_ulp=0, n_pix=0):
    """[rmse, medae, ssim, psnr] under the module docstring's bounds; NaN must meet NaN.  The RMSE bound follows the worst case of
    a sum of ``n_pix`` fp64 terms taken in another order, N * 2^-53 relative, and 1e-10 is that bound's round value at the real
    frame's 67,980 pixels.  The worst case grows with N -- 5.8e-11 at 8 x 65,600 pixels and 2.3e-10 at 8 x 262,160, the two sizes
    that make the kernels stride (tests/meters_ref.py), the second already past 1e-10 -- so the bound is
    max(1e-10, 4 * N * 2^-53): 2.3e-10 and 9.3e-10 at those two, and 1e-10, unchanged, wherever N is below 225,000 pixels (every
    earlier case, and every caller that passes no ``n_pix``)."""
    rmse_tol = max(1e-10, 4 * n_pix * 2.0 ** -53)
    with np.errstate(invalid="ignore"):  # (inf - inf where both are +inf)
        print(f"{tag}: got {got!r} want {want!r} diff {np.abs(got - want)!r}")
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    rmse, medae, ssim, psnr = got
    if not np.isnan(want[0]):
        assert abs(rmse - want[0]) <= rmse_tol * abs(want[0]), tag
    if not np.isnan(want[1]):
        if medae_ulp:
            assert abs(medae - want[1]) <= medae_ulp * EPS64 * abs(want[1]), tag
        else:
            assert medae == want[1], tag
    if not np.isnan(want[2]):
        assert abs(ssim - want[2]) <= 1e-9, tag
    if not np.isnan(want[3]):
        assert psnr == want[3] or abs(psnr - want[3]) <= 1e-9, tag  # (== : both +inf for identical images)


def _check_meter(got, want, tag=""):
    """measure() = [rmse, medae, lpips, ssim, psnr], a mean over updates, against the mean of the restatement's rows."""
    assert got.dtype == np.float64 and got.shape == (5,)
    assert np.isnan(got[2]) == np.isnan(want[2]) and (np.isnan(want[2]) or abs(got[2] - want[2]) <= 4 * EPS64 * abs(want[2]))
    _check_row(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]], tag, medae_ulp=4)


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_image_errors_vs_float64_restatement(name):
    pred, gt, hi, want = _case(name)
    got = _device_errors(pred, gt, ref.LO, hi)
    _check_row(got, want, name, n_pix=pred.size)
    # the median against numpy directly, as float32 bits
    d = np.abs(ref.clamp32(gt, ref.LO, hi) - ref.clamp32(pred, ref.LO, hi))
    assert np.float32(got[1]).tobytes() == np.float32(np.median(d)).tobytes() and got[1] == float(np.float32(got[1]))
    if name.endswith("_ties"):
        assert got[1] == 0.0


def test_one_nan_pixel_makes_every_output_nan():
    pred, gt = ref.make_pair(16, 16, 80.0, 0.3, 0.1, 1)
    pred[5, 7] = np.nan
    assert np.isnan(ref.errors_f64(pred, gt, ref.LO, 80.0)).all()
    assert np.isnan(_device_errors(pred, gt, ref.LO, 80.0)).all()
    pred, gt = ref.make_pair(16, 16, 80.0, 0.3, 0.1, 1)
    gt[15, 15] = np.nan  # a corner: inside one window only
    assert np.isnan(_device_errors(pred, gt, ref.LO, 80.0)).all()


def test_constant_ground_truth_gives_the_formulas_ieee_result():
    """R = 0: C1 = C2 = 0 and the ground truth's variance is 0; whatever the formula gives in IEEE arithmetic (0/0 is NaN)."""
    pred, _ = ref.make_pair(9, 9, 80.0, 0.0, 0.0, 2)
    gt = np.full((9, 9), 20.0, dtype=np.float32)
    want = ref.errors_f64(pred, gt, ref.LO, 80.0)
    _check_row(_device_errors(pred, gt, ref.LO, 80.0), want, "constant gt")
    want = ref.errors_f64(gt, gt, ref.LO, 80.0)  # and a constant prediction as well: 0/0 in every window
    assert np.isnan(want[2]) and want[0] == 0.0 and want[3] == np.inf
    _check_row(_device_errors(gt, gt, ref.LO, 80.0), want, "constant both")


def test_two_calls_are_bit_identical():
    pred, gt, hi, _ = _case("66x1030")
    a, b = _device_errors(pred, gt, ref.LO, hi), _device_errors(pred, gt, ref.LO, hi)
    assert a.tobytes() == b.tobytes()


def test_too_small_an_image_is_an_error_status_with_a_message():
    from lidar4d_amd import _eval_lib, ops
    from lidar4d_amd.metrics import image_errors
    x = torch.rand(6, 40, device=DEV)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    status = _eval_lib.lib().l4de_image_errors(ops._p(x), ops._p(x), 6, 40, 0.0, 1.0, ops._p(out), ops._p(ws), ops._stream())
    assert status != 0 and b"at least 7" in _eval_lib.lib().l4de_last_error()
    with pytest.raises(_eval_lib.HipExtensionError, match="at least 7"):
        image_errors(x, x, 0.0, 1.0)
    with pytest.raises(_eval_lib.HipExtensionError):
        image_errors(x.T.contiguous(), x.T.contiguous(), 0.0, 1.0)  # W = 6


# ---- the meters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["depth", "intensity"])
def test_meter_mean_over_updates_lpips_slot_and_untouched_inputs(kind):
    from lidar4d_amd.metrics import DepthMeter, IntensityMeter
    cls, scale, hi = (DepthMeter, 0.0125, 80.0) if kind == "depth" else (IntensityMeter, 1.0, 1.0)
    pairs = [ref.make_pair(33, 70, hi, 0.3, 0.1, seed) for seed in (0, 1)]
    meter, want = cls(scale), ref.RefMeter(ref.LO, hi)
    for pred, gt in pairs:
        p = torch.from_numpy(pred).to(DEV)[None] * scale
        g = torch.from_numpy(gt).to(DEV)[None] * scale
        p0, g0 = p.clone(), g.clone()
        meter.update(p, g)
        assert torch.equal(p, p0) and torch.equal(g, g0)                 # the reference clamps host copies; nothing here is modified
        want.update((p / scale)[0].cpu().numpy(), (g / scale)[0].cpu().numpy())
    assert meter.N == 2 and all(v.is_cuda and v.dtype == torch.float64 and v.shape == (5,) for v in meter.V)
    got = meter.measure()
    assert np.isnan(got[2])
    _check_meter(got, want.measure(), kind)
    for v, row in zip(meter.V, want.rows):                               # every update on its own: the median bit-equal
        _check_row(v.cpu().numpy()[[0, 1, 3, 4]], row[[0, 1, 3, 4]], kind)
    label = "Depth_error" if kind == "depth" else "Inten_error"
    assert meter.report() == f"{label} = {got}"
    meter.clear()
    assert meter.N == 0 and meter.V == []
    # a caller's LPIPS lands in slot 2 and sees the CLAMPED [H, W] images
    seen = []

    def lpips_stub(a, b, normalize=False):
        seen.append((a, b, normalize))
        return torch.tensor([[[[0.25]]]], device=a.device)

    meter = cls(scale, lpips_fn=lpips_stub)
    pred, gt = pairs[0]
    meter.update(torch.from_numpy(pred).to(DEV)[None] * scale, torch.from_numpy(gt).to(DEV)[None] * scale)
    got = meter.measure()
    assert got[2] == 0.25 and not np.isnan(got[[0, 1, 3, 4]]).any()
    a, b, normalize = seen[0]
    assert normalize is True and a.shape == (33, 70) and b.shape == (33, 70)
    assert float(a.min()) == float(np.float32(1e-6)) and float(a.max()) == hi and float(b.min()) == float(np.float32(1e-6))
    with pytest.raises(ValueError):
        meter.update(torch.zeros(2, 33, 70, device=DEV), torch.zeros(2, 33, 70, device=DEV))
    with pytest.raises(ValueError):
        meter.update(torch.zeros(33, 70, device=DEV), torch.zeros(33, 70, device=DEV))


# ---- Trainer.evaluate --------------------------------------------------------------------------------------------------------------
def test_trainer_evaluate_equals_meters_fed_the_same_predictions_and_restores_the_weights():
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.metrics import PointsMeter, RaydropMeter
    from lidar4d_amd.trainer import Trainer
    from oracle.make_golden import SMALL_MODEL
    torch.manual_seed(0)
    H, W = 16, 64
    data = SyntheticKitti360(DEV, H=H, W=W, num_frames=3, num_rays=256)
    model = LiDAR4D(**dict(SMALL_MODEL, num_frames=3, near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE)).to(DEV)
    tr = Trainer(model, data, num_steps=64, iters=100, chamfer=False, flow=False, ema_decay=0.95, epoch_steps=1, init_scale=1.0)
    for k in range(3):
        tr.train_step(data.batch_for(k))  # three epochs: the EMA moves away from the raw weights
    flat = model._store.flat
    assert tr.ema.num_updates == 3 and not torch.equal(tr.ema.shadow, flat)
    before = flat.detach().clone()

    # Two forward passes of the same frame on the same weights need not be bit-equal on the device (the U-Net's convolutions go
    # through MIOpen, whose first call of a shape searches and may run another solver than later calls), and the meters'
    # bounds are far below fp32 rounding.  So the restatement is fed the very tensors evaluate() received from test_step, and
    # those tensors are pinned to the EMA weights from both sides: a second test_step on the EMA weights reproduces them to
    # REPEAT_TOL, a test_step on the raw weights is at least ten times that away.
    # REPEAT_TOL = 1e-4 absolute on values of order 1: fp32 rounding (6e-8) of reductions over up to about a thousand terms
    # (64 samples per ray, then the U-Net's 3x3 convolutions over up to 128 channels) in another order.
    REPEAT_TOL = 1e-4
    seen = []
    inner = tr.test_step

    def recording_test_step(data, **kw):
        out = inner(data, **kw)
        seen.append((kw, tuple(t.detach().clone() for t in out)))
        return out

    tr.test_step = recording_test_step
    try:
        res = tr.evaluate()
    finally:
        del tr.test_step

    assert torch.equal(flat, before) and tr.ema.backup is None           # bit-equal arena: the raw weights are back
    assert set(res) == {"loss", "raydrop", "intensity", "depth", "points", "report"}
    assert isinstance(res["loss"], float) and np.isfinite(res["loss"])
    assert len(res["report"]) == 4 and [r.split(" ")[0] for r in res["report"]] == ["Rdrop_error", "Inten_error", "Depth_error", "CD"]
    assert len(seen) == 3 and all(kw.get("alpha_r") == 0 and kw.get("refine") is True for kw, _ in seen)   # unmasked, refined
    was_training = model.training
    model.eval()
    tr.ema.store(), tr.ema.copy_to()
    raydrop, points = RaydropMeter(0.5), PointsMeter(scale=data.scale, intrinsics=data.fov)
    inten, depth = ref.RefMeter(ref.LO, 1.0), ref.RefMeter(ref.LO, 80.0)
    loss, kept = 0.0, 0.0
    for k in range(3):
        fr = data.frame(k)
        rd, ri, dep = seen[k][1]
        again = tr.test_step(fr, refine=True, alpha_r=0)
        assert [t.shape for t in again] == [rd.shape, ri.shape, dep.shape] == [(1, H, W)] * 3
        diffs = [float((a - b).abs().max()) for a, b in zip(again, (rd, ri, dep))]
        print(f"frame {k}: a second forward pass on the EMA weights differs by {diffs} (ray-drop, intensity, depth)")
        assert max(diffs) <= REPEAT_TOL, (k, diffs)
        gt = fr["images_lidar"]
        gt_rd, gt_i, gt_d = gt[..., 0], gt[..., 1] * gt[..., 0], gt[..., 2] * gt[..., 0]
        mask = (rd > 0.5).to(ri.dtype)
        kept += float(mask.mean()) / 3
        loss += float(((dep * mask - gt_d).abs().mean() + 0.01 * ((rd - gt_rd) ** 2).mean() + 0.1 * ((ri * mask - gt_i) ** 2).mean())) / 3
        raydrop.update(rd, gt_rd)
        inten.update(((ri * mask) / 1.0)[0].cpu().numpy(), (gt_i / 1.0)[0].cpu().numpy())
        depth.update(((dep * mask) / data.scale)[0].cpu().numpy(), (gt_d / data.scale)[0].cpu().numpy())
        points.update(dep * mask, gt_d)
    tr.ema.restore()
    assert torch.equal(flat, before)
    for k in range(3):  # the raw weights render something else: evaluate() did swap the EMA in
        raw = tr.test_step(data.frame(k), refine=True, alpha_r=0)
        diffs = [float((a - b).abs().max()) for a, b in zip(raw, seen[k][1])]
        print(f"frame {k}: the raw weights' predictions differ from the evaluated ones by {diffs}")
        assert max(diffs) > 10 * REPEAT_TOL, (k, diffs)
    model.train(was_training)
    print(f"predicted keep fraction {kept:.3f}, loss {res['loss']:.6f} vs {loss:.6f}")
    assert abs(res["loss"] - loss) <= 1e-5 * abs(loss)
    # the two meters that were here before, fed the same tensors: fp64 sums (ray-drop) and fp32 means of the chamfer distances
    # (points) whose order the library does not promise
    np.testing.assert_allclose(res["raydrop"], raydrop.measure(), rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(res["points"], points.measure(), rtol=1e-6, atol=0, equal_nan=True)
    _check_meter(res["intensity"], inten.measure(), "intensity")
    _check_meter(res["depth"], depth.measure(), "depth")
    assert res["report"][2] == f"Depth_error = {res['depth']}"
    # a subset of frames, without an EMA and without the U-Net
    tr.ema = None
    one = tr.evaluate(frames=[1], refine=False)
    assert torch.equal(flat, before) and one["depth"].shape == (5,) and np.isnan(one["depth"][2])
