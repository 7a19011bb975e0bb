"""CPU tests of the fused line-of-sight loss (lidar4d_amd.trainer.line_of_sight_loss, include/lidar4d_loss.h): the fourth shared
object's argument checks (its C ABI: tests/test_abi_cpu.py), the absence of a CPU path, and that a
Trainer without ``fused_urf`` keeps the torch route (tests/test_gpu_los.py compares the kernels with it)."""
import pytest
import torch


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
