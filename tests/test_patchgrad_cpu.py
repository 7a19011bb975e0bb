"""CPU tests of the fused patch depth-gradient loss (lidar4d_amd.trainer.patch_depth_grad_loss, include/lidar4d_patch.h): the
fifth shared object's argument checks (its C ABI: tests/test_abi_cpu.py), the absence of a CPU path, that a Trainer without ``fused_patch`` keeps the torch route, the patch-epoch schedule, and
that the shared case generator (tests/patchgrad_cases.py) makes the cases tests/test_gpu_patchgrad.py relies on."""
import itertools

import pytest
import torch

import patchgrad_cases as pc
import test_abi_cpu as abi


# Kept under their earlier names, as calls of the checks in tests/test_abi_cpu.py, which run there for every library: a new library
# adds no test of this kind.
def test_patch_ctypes_signatures_match_header_prototypes():
    abi.test_ctypes_signatures_match_header_prototypes(abi.ROW["patch"])


def test_patch_library_exports_no_name_of_another():
    abi.test_no_library_exports_a_name_of_another()


def test_workspace_and_argument_checks_need_no_device():
    from lidar4d_amd import _patch_lib
    lib = _patch_lib.lib()
    ws = lib.l4dg_patch_workspace
    assert ws(0, 2, 8) == 0 and ws(-1, 2, 8) == 0 and ws(4, 1, 8) == 0 and ws(4, 8, 1) == 0 and ws(4, 33, 32) == 0
    assert ws(1, 2, 2) > 0 and ws(1024, 2, 8) % 8 == 0 and ws(1, 32, 32) > 0 and ws(1 << 30, 2, 2) == 0
    fwd = lambda n_patch, px, py, kind=0, flags=_patch_lib.GRAD_LOSS, half=0: _patch_lib.call(
        "l4dg_patch_fwd", None, None, None, half, n_patch, px, py, 1.0, kind, flags, 0.1, 0.1, 0.1, 0.1, None, None, None, None)
    with pytest.raises(_patch_lib.HipExtensionError, match="l4dg_patch_fwd.*at most 1024"):
        fwd(4, 33, 32)
    with pytest.raises(_patch_lib.HipExtensionError, match="l4dg_patch_fwd.*n_patch must be at least 1"):
        fwd(0, 2, 8)
    with pytest.raises(_patch_lib.HipExtensionError, match="l4dg_patch_fwd.*at least 2"):
        fwd(4, 1, 8)
    with pytest.raises(_patch_lib.HipExtensionError, match="l4dg_patch_fwd.*null pointer"):
        fwd(4, 2, 8)
    with pytest.raises(_patch_lib.HipExtensionError, match="unknown kind"):
        fwd(4, 2, 8, kind=4)
    with pytest.raises(_patch_lib.HipExtensionError, match="forward differences"):
        fwd(4, 2, 8, flags=_patch_lib.GRAD_LOSS | _patch_lib.SOBEL, half=1)
    with pytest.raises(_patch_lib.HipExtensionError, match="l4dg_patch_bwd.*null pointer"):
        _patch_lib.call("l4dg_patch_bwd", None, None, 16, None, None)
    with pytest.raises(_patch_lib.HipExtensionError, match="l4dg_patch_bwd.*at least 1"):
        _patch_lib.call("l4dg_patch_bwd", None, None, 0, None, None)


def test_patch_depth_grad_loss_has_no_cpu_fallback():
    from lidar4d_amd import _lib
    from lidar4d_amd.trainer import patch_depth_grad_loss
    c = pc.make("6x2x8")
    with pytest.raises(_lib.HipExtensionError):
        patch_depth_grad_loss(c["pred"].requires_grad_(True), c["gt"], c["hit"], [2, 8], c["scale"])
    # ... and what it decides before it needs the device
    assert float(patch_depth_grad_loss(c["pred"], c["gt"], c["hit"], 1, c["scale"])) == 0.0  # single pixels: a zero, like depth_grad_loss


@pytest.mark.gpu
def test_patch_depth_grad_loss_argument_errors():
    """The ValueErrors are raised for tensors that are on the device (a CPU tensor is refused first)."""
    from lidar4d_amd.trainer import patch_depth_grad_loss
    c = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in pc.make("6x2x8").items()}
    with pytest.raises(ValueError, match="whole number"):
        patch_depth_grad_loss(c["pred"], c["gt"], c["hit"], [2, 5], c["scale"])
    with pytest.raises(ValueError, match="1024"):
        patch_depth_grad_loss(c["pred"].repeat(1, 11), c["gt"].repeat(1, 11), c["hit"].repeat(1, 11), [33, 32], c["scale"])
    with pytest.raises(ValueError, match="unknown kind"):
        patch_depth_grad_loss(c["pred"], c["gt"], c["hit"], [2, 8], c["scale"], kind="bce")


class _OracleChamfer:
    """chamfer_3DDist stand-in on the CPU: the oracle's brute force (the product's operator is HIP-only)."""

    def __call__(self, a, b):
        from oracle import chamfer_ref
        return chamfer_ref.chamfer(a, b)


def test_bare_trainer_keeps_the_torch_route(monkeypatch):
    """A Trainer object without the ``fused_patch`` attribute (tests/train_golden.py builds one with object.__new__) takes
    ``depth_grad_loss`` with today's defaults and reproduces the reference's train_step on the CPU; the fused node is not entered."""
    from tests import train_golden
    import lidar4d_amd.chamfer as chamfer_mod
    from lidar4d_amd import trainer as T
    monkeypatch.setattr(chamfer_mod, "chamfer_3DDist", _OracleChamfer)

    def refuse(*a, **k):
        raise AssertionError("patch_depth_grad_loss entered by a Trainer without fused_patch")

    monkeypatch.setattr(T, "patch_depth_grad_loss", refuse)
    c = train_golden.load("patch_l1")
    assert train_golden.opt_of(c)["patch_size_lidar"] != 1
    loss, leaves = train_golden.evaluate(c, compute_loss=True)
    train_golden.check(c, loss, leaves)


def _stub_trainer(patch_size_lidar=1, **attrs):
    from lidar4d_amd.trainer import Trainer
    tr = object.__new__(Trainer)
    tr.reducer, tr.urf = None, False
    tr.dataset = type("D", (), dict(batch_for=None, next_frame=None, patch_size_lidar=patch_size_lidar))()
    tr.model = type("M", (), dict(_store=type("S", (), dict(flat=type("F", (), dict(is_cuda=True))()))()))()
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


def test_fused_patch_is_what_lets_a_patch_step_be_captured():
    assert _stub_trainer(1).graphs_supported()
    for patch in ([2, 8], 3):
        tr = _stub_trainer(patch)
        assert not tr.graphs_supported()      # a bare Trainer: the torch route
        tr.fused_patch = False
        assert not tr.graphs_supported()
        tr.fused_patch = True
        assert tr.graphs_supported()
    # a Trainer that alternates needs the fused node in its patch epochs, whatever the dataset holds right now
    assert not _stub_trainer(1, change_patch_size_lidar=[2, 8], fused_patch=False).graphs_supported()
    assert _stub_trainer(1, change_patch_size_lidar=[2, 8], fused_patch=True).graphs_supported()


class _RecordingDataset:
    """Records every write of ``patch_size_lidar`` and the value in place when a batch is drawn."""
    num_rays, num_frames, scale = 64, 4, 1.0

    def __init__(self):
        self.__dict__["writes"] = []
        self.__dict__["seen"] = []
        self.__dict__["patch_size_lidar"] = "untouched"

    def __setattr__(self, name, value):
        if name == "patch_size_lidar":
            self.writes.append(value)
        self.__dict__[name] = value

    def batch(self):
        self.seen.append(self.patch_size_lidar)
        return {}


def _schedule_trainer(change, epoch_steps=3, every=2):
    from lidar4d_amd.trainer import Trainer
    tr = object.__new__(Trainer)
    tr.dataset, tr.local_step, tr.epoch_steps, tr.ema = _RecordingDataset(), 0, epoch_steps, None
    tr.change_patch_size_lidar, tr.change_patch_size_epoch = change, every
    tr._step_device_work = lambda data: 0.0
    return tr


def test_patch_epoch_schedule():
    """epoch = local_step // epoch_steps + 1 counts from 1; patches while epoch % change_patch_size_epoch == 0 (runner.py:697-705)."""
    P = [2, 8]
    tr = _schedule_trainer(P)
    for _ in range(12):
        tr.train_step()
    assert tr.dataset.seen == [1, 1, 1, P, P, P, 1, 1, 1, P, P, P]
    tr = _schedule_trainer(3, epoch_steps=2, every=3)
    for _ in range(8):
        tr.train_step()
    assert tr.dataset.seen == [1, 1, 1, 1, 3, 3, 1, 1]
    tr = _schedule_trainer(None)
    for _ in range(7):
        tr.train_step()
    assert tr.dataset.writes == [] and tr.dataset.seen == ["untouched"] * 7
    bare = _schedule_trainer(None)
    del bare.change_patch_size_lidar, bare.change_patch_size_epoch  # (a Trainer object from before the option)
    bare.train_step()
    assert bare.dataset.writes == []


def test_trainer_refuses_rays_that_are_no_whole_patches(monkeypatch):
    from lidar4d_amd import trainer as T
    model = type("M", (), dict(_store=type("S", (), dict(flat=torch.zeros(1)))()))()
    monkeypatch.setattr(T, "FlatAdam", lambda *a, **k: (_ for _ in ()).throw(AssertionError("constructed past the check")))
    data = type("D", (), dict(num_rays=100, num_frames=3, scale=1.0))()
    with pytest.raises(ValueError, match="whole number of 2 x 8 patches"):
        T.Trainer(model, data, flow=False, change_patch_size_lidar=[2, 8])
    with pytest.raises(ValueError, match="whole number of 3 x 3 patches"):
        T.Trainer(model, data, flow=False, change_patch_size_lidar=3)
    with pytest.raises(ValueError, match="depth_grad_loss"):
        T.Trainer(model, data, flow=False, depth_grad_loss="bce")


# ---- the generator makes the cases it is meant to (conditions on the inputs: the restatement alone, before any GPU run) ----------
@pytest.mark.parametrize("name", pc.MULTI_PATCH)
def test_generator_masks_go_both_ways(name):
    c = pc.make(name)
    m = pc.mask_of(c)
    assert float(m.mean()) >= 0.25 and float(1 - m.mean()) >= 0.25, float(m.mean())
    q = c["gt"].reshape(c["n_patch"], c["px"], c["py"]) / c["scale"]
    d = (q[:, :, :-1] - q[:, :, 1:]).abs()
    assert not bool(((d > 0.005) & (d < 0.02)).any())  # clear of the 0.01 threshold on both sides
    if name in ("6x2x8", "8x3x3"):  # the cases the Sobel cross runs on: interior responses on both sides, borders far beyond
        cs = pc.make(name, scale=pc.SCALE_POW2)
        ms = pc.mask_of(cs, sobel=True)
        assert 0 < int(ms.sum()) < ms.numel()


@pytest.mark.parametrize("name", pc.MULTI_PATCH)
def test_generator_takes_both_huber_branches(name):
    from lidar4d_amd.trainer import _patch_grads
    for scale in (pc.KITTI360_SCALE, pc.SCALE_POW2):
        c = pc.make(name, scale=scale)
        n, px, py = c["n_patch"], c["px"], c["py"]
        pgx = _patch_grads(c["pred"].reshape(n, 1, px, py) / scale, False)[0].abs().reshape(n, px, py - 1)
        ggx = _patch_grads(c["gt"].reshape(n, 1, px, py) / scale, False)[0].reshape(n, px, py - 1)
        m = pc.mask_of(c)
        z = ((pgx - ggx) * m).abs()[m > 0]
        delta = 0.2 * scale
        assert int((z < delta).sum()) >= 3 and int((z >= delta).sum()) >= 3, (name, scale, int((z < delta).sum()), int((z >= delta).sum()))


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("name", pc.MULTI_PATCH)
def test_generator_gives_every_kind_a_value_and_a_gradient(name, kind):
    from lidar4d_amd.trainer import depth_grad_loss
    loss, g = pc.run(depth_grad_loss, pc.make(name, flat=kind != "cos"), kind=kind)
    assert float(loss) > 0.0 and float(g.abs().max()) > 0.0 and bool(torch.isfinite(g).all())


def test_generator_plants():
    from lidar4d_amd.trainer import depth_grad_loss
    c = pc.make("6x2x8")
    view = lambda t: t.reshape(6, 2, 8)
    assert float(view(c["hit"])[pc.ALL_DROPPED].abs().max()) == 0.0 and float(view(c["pred"])[pc.ALL_DROPPED].abs().max()) == 0.0
    assert torch.equal(view(c["pred"])[pc.EXACT], view(c["gt"])[pc.EXACT]) and float(pc.mask_of(c)[pc.EXACT].min()) == 1.0
    flat = view(c["pred"])[pc.FLAT][view(c["hit"])[pc.FLAT] > 0]
    assert flat.numel() >= 8 and float(flat.max()) == float(flat.min()) > 0.0
    assert not torch.equal(view(pc.make("6x2x8", flat=False)["pred"])[pc.FLAT], view(c["pred"])[pc.FLAT])
    _, g = pc.run(depth_grad_loss, c)
    assert float(view(g)[pc.ALL_DROPPED].abs().max()) == 0.0 and float(view(g)[pc.EXACT].abs().max()) == 0.0  # ties: gradient 0
    h = pc.make("8x3x3", half=True)
    assert h["gt"].dtype == torch.float16 and h["hit"].dtype == torch.float16 and h["pred"].dtype == torch.float32
    assert sorted(pc.CASES) == sorted(["1x2x2", "6x2x8", "8x3x3", "4x4x8", "3x8x16", "300x2x8", "1x32x32"])
    assert len(set(itertools.chain.from_iterable(pc.shape_of(k)[1:] for k in pc.CASES))) >= 5
