"""CPU tests of the evaluation meters (lidar4d_amd/metrics.py DepthMeter / IntensityMeter, include/lidar4d_eval.h): the third
shared object's argument checks (its C ABI: tests/test_abi_cpu.py), the absence of a CPU path, and the numpy restatements
tests/test_gpu_meters.py compares the kernels with (tests/meters_ref.py): the float64 formula against plain loops and against the
reference's own float32 arithmetic."""
import numpy as np
import pytest
import torch

import meters_ref as ref


def test_workspace_and_argument_checks_need_no_device():
    from lidar4d_amd import _eval_lib
    lib = _eval_lib.lib()
    assert lib.l4de_image_errors_workspace(6, 100) == 0 and lib.l4de_image_errors_workspace(100, 6) == 0
    assert lib.l4de_image_errors_workspace(66, 1030) >= 66 * 1030 * 4
    assert lib.l4de_image_errors_workspace(7, 7) % 8 == 0
    with pytest.raises(_eval_lib.HipExtensionError, match="at least 7"):
        _eval_lib.call("l4de_image_errors", None, None, 6, 64, 0.0, 1.0, None, None, None)


# ---- no CPU path ---------------------------------------------------------------------------------------------------------------
def test_meters_have_no_cpu_fallback():
    from lidar4d_amd import _lib
    from lidar4d_amd.metrics import DepthMeter, IntensityMeter
    cpu = torch.rand(1, 16, 16)
    for meter in (DepthMeter(1.0), IntensityMeter(1.0)):
        with pytest.raises(_lib.HipExtensionError):
            meter.update(cpu, cpu)
        assert meter.N == 0 and meter.V == []
        with pytest.raises(ValueError):
            meter.update(torch.rand(2, 16, 16), torch.rand(2, 16, 16))
    assert DepthMeter(0.5).scale == 0.5 and DepthMeter(1.0, lpips_fn=len).lpips_fn is len
    assert (DepthMeter.lo, DepthMeter.hi) == (1e-6, 80.0) and (IntensityMeter.lo, IntensityMeter.hi) == (1e-6, 1.0)


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def test_generator_makes_the_cases_it_is_meant_to():
    pred, gt = ref.make_pair(*ref.CASES["66x1030"])
    assert pred.dtype == gt.dtype == np.float32 and pred.shape == (66, 1030)
    assert pred.min() == -1.0 and pred.max() == 160.0 and gt.min() == -1.0 and gt.max() == 160.0  # both clamps, both images
    assert np.array_equal(ref.make_pair(*ref.CASES["66x1030"])[0], pred)                          # deterministic
    pred, gt = ref.make_pair(*ref.CASES["66x1030_ties"])
    d = np.abs(ref.clamp32(gt, ref.LO, 80.0) - ref.clamp32(pred, ref.LO, 80.0))
    assert np.count_nonzero(d == 0) > d.size // 2 and ref.errors_f64(pred, gt, ref.LO, 80.0)[1] == 0.0
    H, W = ref.CASES["8x9"][:2]
    assert (H * W) % 2 == 0 and (ref.CASES["7x7"][0] * ref.CASES["7x7"][1]) % 2 == 1


def test_identical_images_score_one_and_zero():
    pred, gt = ref.make_pair(*ref.CASES["33x70_intensity"])
    with np.errstate(divide="ignore"):
        rmse, medae, ssim, psnr = ref.errors_f64(gt, gt, ref.LO, 1.0)
    assert rmse == 0.0 and medae == 0.0 and psnr == np.inf
    assert abs(ssim - 1.0) <= 1e-12


def test_clamp_keeps_nan_and_median_is_nan_then():
    x = np.array([[np.nan, -1.0, 0.5, 3.0]], dtype=np.float32)
    c = ref.clamp32(x, ref.LO, 1.0)
    assert np.isnan(c[0, 0]) and c[0, 1] == np.float32(1e-6) and c[0, 2] == 0.5 and c[0, 3] == 1.0
    pred, gt = ref.make_pair(16, 16, 80.0, 0.3, 0.1, 1)
    pred[5, 7] = np.nan
    assert np.isnan(ref.errors_f64(pred, gt, ref.LO, 80.0)).all()


@pytest.mark.parametrize("case", ["7x7", "8x9"])
def test_float64_formula_against_plain_loops(case):
    H, W, hi = ref.CASES[case][:3]
    pred, gt = ref.make_pair(*ref.CASES[case])
    a, b = ref.errors_f64(pred, gt, ref.LO, hi), ref.errors_loops(pred, gt, ref.LO, hi)
    assert abs(a[2] - b[2]) <= 1e-12 and abs(a[0] - b[0]) <= 1e-12 * b[0] and abs(a[3] - b[3]) <= 1e-10
    # the median by sorting: middle value, or the float32 mean of the two middle values
    d = np.sort(np.abs(ref.clamp32(gt, ref.LO, hi) - ref.clamp32(pred, ref.LO, hi)).ravel())
    n = d.size
    want = d[n // 2] if n % 2 else (d[n // 2 - 1] + d[n // 2]) / np.float32(2)
    assert np.float32(a[1]) == want and a[1] == float(want)


@pytest.mark.parametrize("case", list(ref.CASES))
def test_float64_formula_against_the_references_float32_path(case):
    """errors_f64 (what the kernels implement) against the reference's literal float32 arithmetic.  Bounds: SSIM 1e-5, RMSE
    1e-5 relative, MedAE equal -- about 50 times what float32 rounding gives on these images (the figures are printed) and far
    below a slip in the formula (test_a_slip_in_the_formula_is_outside_the_bound)."""
    H, W, hi = ref.CASES[case][:3]
    pred, gt = ref.make_pair(*ref.CASES[case])
    a, b = ref.errors_f64(pred, gt, ref.LO, hi), ref.errors_ref32(pred, gt, ref.LO, hi)
    print(f"{case}: |d ssim| = {abs(a[2] - b[2]):.3e}, rel d rmse = {abs(a[0] - b[0]) / b[0]:.3e}, d medae = {a[1] - b[1]:.3e}, "
          f"|d psnr| = {abs(a[3] - b[3]):.3e}")
    assert abs(a[2] - b[2]) <= 1e-5
    assert abs(a[0] - b[0]) <= 1e-5 * b[0]
    assert a[1] == b[1]


def test_a_slip_in_the_formula_is_outside_the_bound():
    """Biased instead of sample covariance (49/49 for 49/48) on the real frame moves SSIM by far more than the 1e-5 the
    comparison above allows."""
    hi = ref.CASES["66x1030"][2]
    pred, gt = ref.make_pair(*ref.CASES["66x1030"])
    p, g = ref.clamp32(pred, ref.LO, hi).astype(np.float64), ref.clamp32(gt, ref.LO, hi).astype(np.float64)
    m = ref.window_means_f64
    ux, uy, uxx, uyy, uxy = m(p), m(g), m(p * p), m(g * g), m(p * g)
    R = g.max() - g.min()
    C1, C2 = (ref.K1 * R) ** 2, (ref.K2 * R) ** 2
    biased = np.mean((2 * ux * uy + C1) * (2 * (uxy - ux * uy) + C2) / ((ux * ux + uy * uy + C1) * (uxx - ux * ux + uyy - uy * uy + C2)))
    print(f"biased covariance moves ssim by {abs(biased - ref.errors_f64(pred, gt, ref.LO, hi)[2]):.3e}")
    assert abs(biased - ref.errors_f64(pred, gt, ref.LO, hi)[2]) > 1e-4
