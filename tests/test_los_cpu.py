"""CPU tests of the fused line-of-sight loss (lidar4d_amd.trainer.line_of_sight_loss, include/lidar4d_loss.h): the fourth shared
object's ABI, its loading on first use, the absence of a CPU path, and that a Trainer without ``fused_urf`` keeps the torch
route (tests/test_gpu_los.py compares the kernels with it)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lidar4d_loss.h")


def _declared():
    header = open(HEADER).read()
    return set(re.findall(r"\b(l4dl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def test_loss_library_exports_declared_abi():
    from lidar4d_amd import _eval_lib, _lib, _loss_lib, _prep_lib
    declared = _declared()
    assert declared == set(_loss_lib.SIGNATURES) | {"l4dl_version", "l4dl_last_error"}
    assert set(_loss_lib.SIGNATURES) == {"l4dl_los_workspace", "l4dl_los_fwd", "l4dl_los_bwd"}
    assert os.path.exists(_loss_lib.LIB_PATH), "liblidar4d_loss.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(_loss_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/lidar4d_loss.h but not exported"
    assert _loss_lib.lib().l4dl_version() == _loss_lib.ABI_VERSION == 1
    assert shutil.which("nm"), "needs binutils nm"
    exported = _exported(_loss_lib.LIB_PATH)
    assert exported == declared, (sorted(exported - declared)[:8], declared - exported)
    # ... and the other three libraries gained nothing
    for other in (_lib.LIB_PATH, _prep_lib.LIB_PATH, _eval_lib.LIB_PATH):
        assert not [s for s in _exported(other) if "l4dl_" in s], other


def test_loss_ctypes_signatures_match_header_prototypes():
    """Every prototype of include/lidar4d_loss.h against _loss_lib.SIGNATURES: same number of arguments and the same kind
    (pointer / int32 / int64 / float / double) in every position."""
    from lidar4d_amd import _lib, _loss_lib
    header = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(?:int|int64_t|void\s*\*)\s*(l4dl_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))

    def kind(arg):
        arg = arg.strip()
        if "*" in arg:
            return "ptr"
        for name, k in (("int64_t", "i64"), ("int32_t", "i32"), ("double", "f64"), ("float", "f32"), ("int ", "i32")):
            if arg.startswith(name):
                return k
        raise AssertionError(f"unparsed argument {arg!r}")

    ckind = {_lib.P: "ptr", _lib.I32: "i32", _lib.I64: "i64", _lib.F32: "f32", _lib.F64: "f64"}
    for name, argtypes in _loss_lib.SIGNATURES.items():
        assert name in protos, f"{name} bound but no prototype found"
        args = [a for a in protos[name].split(",") if a.strip() and a.strip() != "void"]
        assert [kind(a) for a in args] == [ckind[t] for t in argtypes], name
        if not name.endswith("_workspace"):
            assert re.match(r"void\s*\*\s*stream$", args[-1].strip()), name  # the stream comes last
    assert set(protos) == set(_loss_lib.SIGNATURES) | {"l4dl_version"}  # (l4dl_last_error returns const char*)


def test_loss_c_abi_from_plain_c(tmp_path):
    from lidar4d_amd import _loss_lib
    assert shutil.which("gcc") and os.path.exists(_loss_lib.LIB_PATH), "needs gcc and the built library"
    exe = str(tmp_path / "loss_abi_check")
    libdir = os.path.dirname(_loss_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "loss_abi_check.c"), "-L", libdir, "-llidar4d_loss", f"-Wl,-rpath,{libdir}",
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith(f"{len(_loss_lib.SIGNATURES) + 2} entry points, ABI v{_loss_lib.ABI_VERSION}")


def test_loss_library_is_loaded_on_first_use_only():
    code = ("import lidar4d_amd, lidar4d_amd.trainer\n"
            "from lidar4d_amd import _loss_lib\n"
            "assert callable(lidar4d_amd.trainer.line_of_sight_loss)\n"
            "assert 'liblidar4d_loss' not in open('/proc/self/maps').read()\n"
            "_loss_lib.lib()\n"
            "assert 'liblidar4d_loss' in open('/proc/self/maps').read()\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_workspace_and_argument_checks_need_no_device():
    from lidar4d_amd import _loss_lib
    lib = _loss_lib.lib()
    assert lib.l4dl_los_workspace(0, 768) == 0 and lib.l4dl_los_workspace(16384, 0) == 0 and lib.l4dl_los_workspace(-1, 4) == 0
    assert lib.l4dl_los_workspace(1, 1) > 0 and lib.l4dl_los_workspace(16384, 768) % 8 == 0
    with pytest.raises(_loss_lib.HipExtensionError, match="at least 1"):
        _loss_lib.call("l4dl_los_fwd", None, None, None, 0, 0, 8, None, 0, 1000, None, None, None)
    with pytest.raises(_loss_lib.HipExtensionError, match="iters"):
        _loss_lib.call("l4dl_los_bwd", None, None, None, 0, 8, 8, None, 0, 0, None, None, None, None)
    with pytest.raises(_loss_lib.HipExtensionError, match="null pointer"):
        _loss_lib.call("l4dl_los_fwd", None, None, None, 0, 8, 8, None, 0, 1000, None, None, None)


def test_line_of_sight_loss_has_no_cpu_fallback():
    from lidar4d_amd import _lib
    from lidar4d_amd.trainer import line_of_sight_loss
    out = {"weights": torch.rand(4, 8, requires_grad=True), "z_vals": torch.rand(4, 8)}
    with pytest.raises(_lib.HipExtensionError):
        line_of_sight_loss(out, torch.rand(1, 4), 0, 1000)
    with pytest.raises(_lib.HipExtensionError):
        line_of_sight_loss(out, torch.rand(1, 4), 0, 1000, sched=torch.tensor([0.0, 1.0]))


class _OracleChamfer:
    """chamfer_3DDist stand-in on the CPU: the oracle's brute force (the product's operator is HIP-only)."""

    def __call__(self, a, b):
        from oracle import chamfer_ref
        return chamfer_ref.chamfer(a, b)


def test_bare_trainer_keeps_the_torch_route(monkeypatch):
    """A Trainer object without the ``fused_urf`` attribute (tests/train_golden.py builds one with object.__new__) takes
    ``urf_loss`` and reproduces the reference's train_step on the CPU; the fused node is not entered."""
    from tests import train_golden
    import lidar4d_amd.chamfer as chamfer_mod
    from lidar4d_amd import trainer as T
    monkeypatch.setattr(chamfer_mod, "chamfer_3DDist", _OracleChamfer)

    def refuse(*a, **k):
        raise AssertionError("line_of_sight_loss entered by a Trainer without fused_urf")

    monkeypatch.setattr(T, "line_of_sight_loss", refuse)
    c = train_golden.load("urf")
    assert bool(train_golden.opt_of(c)["urf_loss"])
    loss, leaves = train_golden.evaluate(c, compute_loss=True)
    train_golden.check(c, loss, leaves)
    assert float(c["g_weights"].abs().max()) > 0.0  # only the line-of-sight term reaches the weights


def test_fused_urf_is_what_lets_the_term_be_captured():
    """graphs_supported() with ``urf=True``: only with ``fused_urf`` (the torch route computes the tolerance on the host)."""
    from lidar4d_amd.trainer import Trainer
    tr = object.__new__(Trainer)
    tr.reducer, tr.urf = None, True
    tr.dataset = type("D", (), dict(batch_for=None, next_frame=None, patch_size_lidar=1))()
    tr.model = type("M", (), dict(_store=type("S", (), dict(flat=type("F", (), dict(is_cuda=True))()))()))()
    assert not tr.graphs_supported()          # a bare Trainer: the torch route computes eps on the host
    tr.fused_urf = True
    assert tr.graphs_supported()
    tr.fused_urf, tr.urf = False, False
    assert tr.graphs_supported()
