"""CPU tests of the evaluation meters (lidar4d_amd/metrics.py DepthMeter / IntensityMeter, include/lidar4d_eval.h): the third
shared object's ABI, the absence of a CPU path, and the numpy restatements tests/test_gpu_meters.py compares the kernels with
(tests/meters_ref.py): the float64 formula against plain loops and against the reference's own float32 arithmetic."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import meters_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lidar4d_eval.h")


# ---- the third shared object -------------------------------------------------------------------------------------------------
def _declared():
    header = open(HEADER).read()
    return set(re.findall(r"\b(l4de_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def test_eval_library_exports_declared_abi():
    from lidar4d_amd import _eval_lib, _lib, _prep_lib
    declared = _declared()
    assert {"l4de_version", "l4de_last_error"} <= declared
    assert declared == set(_eval_lib.SIGNATURES) | {"l4de_version", "l4de_last_error"}
    assert os.path.exists(_eval_lib.LIB_PATH), "liblidar4d_eval.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(_eval_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/lidar4d_eval.h but not exported"
    assert _eval_lib.lib().l4de_version() == _eval_lib.ABI_VERSION == 1
    assert shutil.which("nm"), "needs binutils nm"
    exported = _exported(_eval_lib.LIB_PATH)
    assert exported == declared, (sorted(exported - declared)[:8], declared - exported)
    # ... and the render and point-preparation libraries gained nothing
    for other in (_lib.LIB_PATH, _prep_lib.LIB_PATH):
        assert not [s for s in _exported(other) if "l4de_" in s], other


def test_eval_ctypes_signatures_match_header_prototypes():
    """Every prototype of include/lidar4d_eval.h against _eval_lib.SIGNATURES: same number of arguments and the same kind
    (pointer / int32 / int64 / float / double) in every position."""
    from lidar4d_amd import _eval_lib, _lib
    header = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(?:int|int64_t|void\s*\*)\s*(l4de_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))

    def kind(arg):
        arg = arg.strip()
        if "*" in arg:
            return "ptr"
        for name, k in (("int64_t", "i64"), ("int32_t", "i32"), ("double", "f64"), ("float", "f32"), ("int ", "i32")):
            if arg.startswith(name):
                return k
        raise AssertionError(f"unparsed argument {arg!r}")

    ckind = {_lib.P: "ptr", _lib.I32: "i32", _lib.I64: "i64", _lib.F32: "f32", _lib.F64: "f64"}
    for name, argtypes in _eval_lib.SIGNATURES.items():
        assert name in protos, f"{name} bound but no prototype found"
        args = [a for a in protos[name].split(",") if a.strip() and a.strip() != "void"]
        assert [kind(a) for a in args] == [ckind[t] for t in argtypes], name
    assert set(protos) == set(_eval_lib.SIGNATURES) | {"l4de_version"}  # (l4de_last_error returns const char*)


def test_eval_c_abi_from_plain_c(tmp_path):
    from lidar4d_amd import _eval_lib
    assert shutil.which("gcc") and os.path.exists(_eval_lib.LIB_PATH), "needs gcc and the built library"
    exe = str(tmp_path / "eval_abi_check")
    libdir = os.path.dirname(_eval_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "eval_abi_check.c"), "-L", libdir, "-llidar4d_eval", f"-Wl,-rpath,{libdir}",
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith(f"{len(_eval_lib.SIGNATURES) + 2} entry points, ABI v{_eval_lib.ABI_VERSION}")


def test_eval_library_is_loaded_on_first_use_only():
    code = ("import lidar4d_amd, lidar4d_amd.trainer, lidar4d_amd.metrics\n"
            "from lidar4d_amd import _eval_lib\n"
            "from lidar4d_amd.metrics import DepthMeter, IntensityMeter\n"
            "DepthMeter(1.0), IntensityMeter(1.0)\n"
            "assert hasattr(lidar4d_amd.trainer.Trainer, 'evaluate')\n"
            "assert 'liblidar4d_eval' not in open('/proc/self/maps').read()\n"
            "_eval_lib.lib()\n"
            "assert 'liblidar4d_eval' in open('/proc/self/maps').read()\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


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
