"""CPU tests of training on a preprocessed sequence: the sixth shared object's argument checks (its C ABI: tests/test_abi_cpu.py); ``lidar_loss`` on the fp16 train-step fixture
(tests/golden/train_step_losses_f16.npz: the reference's own train_step on half ground truth) and, again, on the fp32 one;
``process_pointcloud`` on a fp16 split against the reference's clouds; ``KITTI360Dataset``'s trainer protocol; and the schedule
of ``Trainer.train``."""
import numpy as np
import pytest
import torch

import realdata_cases as rc
import test_abi_cpu as abi


# Kept under their earlier names, as calls of the checks in tests/test_abi_cpu.py, which run there for every library: a new library
# adds no test of this kind.
def test_step_ctypes_signatures_match_header_prototypes():
    abi.test_ctypes_signatures_match_header_prototypes(abi.ROW["step"])


def test_step_library_exports_no_name_of_another():
    abi.test_no_library_exports_a_name_of_another()


def test_step_argument_checks_need_no_device():
    from lidar4d_amd import _step_lib
    lib = _step_lib.lib()
    ws = lib.l4ds_primary_losses_workspace
    assert ws(-1) == 0 and ws(0) == 4 and ws(1) == 4 and ws(256) == 4 and ws(257) == 8
    losses = lambda n, kinds=(0, 1, 1): _step_lib.call("l4ds_primary_losses", None, None, None, 0, None, n, *kinds, 1.0, 0.01, 0.1, 0.2,
                                                       0.002, 0.01, None, None, None, None, None, None, None)
    with pytest.raises(_step_lib.HipExtensionError, match="l4ds_primary_losses.*negative ray count"):
        losses(-1)
    for kinds in ((4, 1, 1), (0, -1, 1), (0, 1, 7)):
        with pytest.raises(_step_lib.HipExtensionError, match="l4ds_primary_losses.*unknown criterion"):
            losses(8, kinds)
    with pytest.raises(_step_lib.HipExtensionError, match="l4ds_primary_losses.*null pointer"):
        losses(8)
    with pytest.raises(_step_lib.HipExtensionError, match="l4ds_primary_losses.*null pointer"):
        losses(0)  # (the loss itself is always written)
    batch = lambda n_patch=4, px=1, py=1, H=8, W=32: _step_lib.call("l4ds_ray_batch", None, None, n_patch, px, py, None, 2.0, 26.9, H, W,
                                                                    None, 0, None, None, None, None, None)
    for px, py in ((0, 8), (2, 0), (-1, -1)):
        with pytest.raises(_step_lib.HipExtensionError, match="l4ds_ray_batch.*patch side must be at least 1"):
            batch(px=px, py=py)
    for H, W in ((0, 32), (-3, 32), (8, 0)):
        with pytest.raises(_step_lib.HipExtensionError, match="l4ds_ray_batch.*empty image"):
            batch(H=H, W=W)
    with pytest.raises(_step_lib.HipExtensionError, match="l4ds_ray_batch.*negative patch count"):
        batch(n_patch=-1)
    with pytest.raises(_step_lib.HipExtensionError, match="l4ds_ray_batch.*null pointer"):
        batch()
    batch(n_patch=0)  # nothing to do: no launch, no error


def test_fused_wrappers_have_no_cpu_fallback():
    from lidar4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.HipExtensionError):
        ops.primary_losses_any(z(4), z(4, 2), z(4, 3).half(), z(4, 3), ("l1", "mse", "mse"), 1.0, 0.01, 0.1, 0.2, 0.002, 0.01, False)
    with pytest.raises(_lib.HipExtensionError):
        ops.ray_batch_patches(z(4, dtype=torch.int64), z(4, dtype=torch.int64), (1, 1), torch.eye(4), (2.0, 26.9), 8, 32, z(8, 32, 3))


# ---- the torch restatement on fp16 ground truth -----------------------------------------------------------------------------------
class _OracleChamfer:
    """chamfer_3DDist stand-in on the CPU: the oracle's brute force (the product's operator is HIP-only)."""

    def __call__(self, a, b):
        from oracle import chamfer_ref
        return chamfer_ref.chamfer(a, b)


def test_criterion_takes_half_targets_as_autocast_does():
    """Without the casts: mse and huber raise 'Found dtype Half but expected Float' in backward, bce returns half."""
    from lidar4d_amd.trainer import criterion
    g = torch.Generator().manual_seed(0)
    b16 = torch.rand(32, generator=g).half()
    for kind in ("l1", "mse", "bce", "huber"):
        a = torch.rand(32, generator=g).requires_grad_(True)
        v = criterion(kind, 0.5)(a, b16)
        assert v.dtype == torch.float32
        v.sum().backward()
        a32 = a.detach().clone().requires_grad_(True)
        w = criterion(kind, 0.5)(a32, b16.float())  # fp32 inputs go through unchanged: the same bits as the widened target
        w.sum().backward()
        assert torch.equal(v, w) and torch.equal(a.grad, a32.grad)


@pytest.mark.parametrize("n", rc.PRIMARY_REF_N)
def test_primary_losses_ref_vs_lidar_loss_in_float64(n, monkeypatch):
    """rc.primary_losses_ref -- what tests/test_gpu_realdata.py holds l4ds_primary_losses to, bit for bit -- against
    ``trainer.lidar_loss`` and its autograd in float64 on the same inputs and the same fp32-rounded scalars (``criterion``'s casts
    to float, the autocast policy, are taken out for the float64 evaluation; the expressions stay).  Per-ray outputs: within
    2 fp32 ulps of the float64 value -- each is at most three roundings of 2^-24 relative behind exact operands (a difference of two
    fp32 values, a square or a doubling, a weight; a product and a quotient for the points).  Loss: within
    (3 n + 2) * 2^-24 * sum |terms|, the bound of glue_cases.flow_loss_finish_ref: 3 n - 1 additions in any order, and up to
    three roundings inside a term.  One constant differs between the two evaluations: the kernel takes the upper smoothing target
    1 - smooth in fp32; its rounding error d enters the ray-drop gradient of the rays with a return as 2 alpha_r d and their terms
    as alpha_r (2 |e_r| + d) d, which the two bounds are widened by (d < 2^-25: below 2e-9 on a gradient of 1e-2)."""
    from lidar4d_amd import trainer as T
    F32, F64 = np.float32, np.float64
    plain = {"l1": lambda a, b: (a - b).abs(), "mse": lambda a, b: (a - b) ** 2}
    monkeypatch.setattr(T, "criterion", lambda kind, scale=1.0: plain[kind])
    depth, image, gt, rays_d, S = rc.loss_inputs(n, half=False, seed=n)
    host = [t.numpy() for t in (depth, image, gt, rays_d)]
    ulps = lambda got, want64: np.abs(got.astype(F64) - want64) / np.spacing(np.abs(want64).astype(F32)).astype(F64)
    for smooth, alphas in rc.PRIMARY_REF_SETTINGS:
        ref = rc.primary_losses_ref(*host, *alphas, smooth, S)
        a_d, a_r, a_i, s32, S32 = (float(F32(v)) for v in (*alphas, smooth, S))
        d64, i64 = depth.double()[None].requires_grad_(True), image.double()[None].requires_grad_(True)
        loss = T.lidar_loss({"depth_lidar": d64, "image_lidar": i64}, gt.double()[None], a_d, a_r, a_i, s32, scale=S32)
        loss.backward()
        loss = loss.detach()
        m = gt[:, 0].double()
        d_hi = abs(float(F32(1.0) - F32(smooth)) - (1.0 - s32))
        assert d_hi < 2.0 ** -25 and set(m.tolist()) <= {0.0, 1.0}
        e_r = (image[:, 0].double() - (1.0 - s32)).abs() * m
        bound = (3 * n + 2) * 2.0 ** -24 * float(loss) + a_r * float(((2 * e_r + d_hi) * d_hi * m).sum())
        assert float(loss) > 0 and abs(float(ref["loss"][0]) - float(loss)) <= bound, (n, smooth, float(ref["loss"][0]), float(loss), bound)
        pts64 = torch.stack([rays_d.double() * (depth.double() * m)[:, None] / S32, rays_d.double() * (gt[:, 2].double() * m)[:, None] / S32])
        slack = np.zeros((n, 2))
        slack[:, 0] = 2 * a_r * d_hi * m.numpy()
        for name, want, extra in (("g_depth", d64.grad[0], 0.0), ("g_image", i64.grad[0], slack), ("pts", pts64, 0.0)):
            want = want.numpy()
            off = np.abs(ref[name].astype(F64) - want) - extra
            worst = float((off / np.spacing(np.abs(want).astype(F32)).astype(F64)).max())
            assert ref[name].shape == want.shape and worst <= 2.0, (name, n, smooth, worst)
            assert n < 255 or float(np.abs(want).max()) > 0
        assert np.array_equal(ref["gt32"], host[2])


def test_fixed_order_sum_drops_and_doubles_no_term():
    """rc.fixed_order_sum on its own: exact on integers (as any order is), also where the second stage takes a second turn, and
    on real values within the bound of its longest chain of additions."""
    F32 = np.float32
    r = np.random.RandomState(5)
    ints = r.randint(-8, 9, size=65793).astype(F32)
    assert float(rc.fixed_order_sum(ints)) == float(ints.astype(np.float64).sum())
    assert float(rc.fixed_order_sum(np.zeros(0, F32))) == 0.0 and float(rc.fixed_order_sum(np.array([2.5], F32))) == 2.5
    # thread t of the second stage adds partial[t] and partial[t + 256]: 258 workgroups of one 1.0 each, the last two landing on threads 0 and 1
    v = np.zeros(258 * 256, F32)
    v[::256] = 1.0
    assert float(rc.fixed_order_sum(v)) == 258.0
    x = r.uniform(0.0, 1.0, size=65793).astype(F32)
    exact = float(x.astype(np.float64).sum())
    assert abs(float(rc.fixed_order_sum(x)) - exact) <= 19 * 2.0 ** -24 * exact  # (positive terms, 8 + 2 + 8 additions deep)


@pytest.mark.parametrize("which,tag", rc.ALL_CASES)
def test_lidar_loss_vs_reference_train_step(which, tag, monkeypatch):
    """The torch restatement of the whole loss block against the reference's train_step, at tests/train_golden.py's CPU bound
    (2e-5): every case of the fp16 fixture, and every case of the fp32 one again (the casts left it alone)."""
    import lidar4d_amd.chamfer as chamfer_mod
    monkeypatch.setattr(chamfer_mod, "chamfer_3DDist", _OracleChamfer)
    c = rc.load(which, tag)
    assert c["images"].dtype == (torch.float16 if which == "f16" else torch.float32)
    loss, leaves = rc.train_golden.evaluate(c)
    rc.train_golden.check(c, loss, leaves)


def test_f16_fixture_is_what_the_issue_asks_for():
    from lidar4d_amd.trainer import frame_index
    assert rc.F16_CASES == ["default", "crit_huber_bce_l1", "crit_mse_l1_huber", "depth_bce", "urf", "patch_2x8", "flow_gap"]
    for tag in rc.F16_CASES:
        c = rc.load("f16", tag)
        o = rc.train_golden.opt_of(c)
        m = c["images"][0, :, 0]
        assert 64 <= int(c["n"]) <= 128 and 0 < int(m.sum()) < m.numel()
        delta = 0.2 * float(o["scale"])
        for kind, err in ((o["depth_loss"], c["depth"][0] - (c["images"][0, :, 2] * m).float()),
                          (o["intensity_loss"], c["image"][0, :, 1] - c["images"][0, :, 1].float())):
            if kind == "huber":
                z = err.abs()[m > 0]
                assert int((z < delta).sum()) >= 3 and int((z > delta).sum()) >= 3, (tag, kind)
    gap = rc.load("f16", "flow_gap")
    k = frame_index(gap["time"], int(rc.train_golden.opt_of(gap)["num_frames"]))
    assert gap[f"pc_{k + 1}"].shape[0] == 0 and gap[f"pc_{k - 1}"].shape[0] > 0 and gap[f"pc_{k}"].shape[0] > 0


# ---- process_pointcloud on a fp16 split --------------------------------------------------------------------------------------------
def test_process_pointcloud_f16_vs_reference(tmp_path, monkeypatch):
    """trainer.process_pointcloud on the fixture sequence's ``refine`` split with fp16 ground truth against the reference's
    process_pointcloud: the same keys (the frames' places in the 51-frame sequence), the same number of points either side of
    the split, and the points to ``bound`` below.  The device conversion is HIP-only; its CPU restatement oracle.convert_ref
    (pinned to the reference bit for bit by tests/test_next_rows.py::test_convert_oracle_pinned_to_reference) stands in, so what
    is under test is the half arithmetic in front of it and the transform behind it."""
    from lidar4d_amd import convert, trainer
    from oracle import convert_ref
    to_points = lambda pano, K: torch.from_numpy(convert_ref.pano_to_lidar_with_intensities(
        pano.numpy().astype(np.float32), np.zeros(tuple(pano.shape), np.float32), K)[:, :3].astype(np.float32))
    monkeypatch.setattr(convert, "pano_to_lidar", to_points)
    keys, clouds, grounds, z0 = rc.pointcloud_fixture()
    ds = rc.fixture_dataset(tmp_path, "refine")
    assert ds.images_lidar.dtype == torch.float16 and keys == [1, 4, 7, 10]
    pc, ground = trainer.process_pointcloud(ds, removal=rc.split_on_z(z0))
    assert list(pc) == [str(k) for k in keys] == list(ground)
    # bound: the conversion stand-in is bit-exact, so what is left is the transform -- fp32 here, float64 in the reference's numpy
    # (three products and three additions per coordinate, each rounded to fp32: 6 * 2^-24 of the largest term) -- on top of the
    # 3e-7 * 80 m (in scene units) tests/test_next_rows.py::test_pano_to_lidar_gpu allows the conversion itself
    for k in keys:
        for got, want in ((pc[str(k)], clouds[k]), (ground[str(k)], grounds[k])):
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and want.shape[0] >= 8
            bound = 3e-7 * 80 * ds.scale + 6 * 2.0 ** -24 * float(np.abs(want).max())
            assert float(np.abs(got.numpy().astype(np.float64) - want).max()) <= bound, (k, bound)


def test_process_pointcloud_reads_either_attribute_pair(monkeypatch):
    from lidar4d_amd import convert, trainer
    g = torch.Generator().manual_seed(1)
    cloud = torch.randn(20, 3, generator=g)
    monkeypatch.setattr(convert, "pano_to_lidar", lambda pano, K: cloud)
    images, poses = torch.rand(2, 4, 8, 3, generator=g), torch.eye(4).repeat(2, 1, 1)
    a = type("A", (), dict(num_frames=2, scale=0.5, fov=(2.0, 26.9), images=images, poses=poses))()
    b = type("B", (), dict(num_frames=51, scale=0.5, fov=(2.0, 26.9), images_lidar=images, poses_lidar=poses,
                           frames=lambda self: range(2), sequence_index=lambda self, k: (3, 9)[k]))()
    pa, ga = trainer.process_pointcloud(a)
    pb, gb = trainer.process_pointcloud(b)
    assert list(pa) == ["0", "1"] and list(pb) == ["3", "9"]
    assert torch.equal(pa["1"], pb["9"]) and torch.equal(ga["0"], gb["3"])


# ---- the dataset protocol ------------------------------------------------------------------------------------------------------------
def test_kitti360_dataset_protocol(tmp_path):
    from torch.utils.data import RandomSampler
    from lidar4d_amd.trainer import frame_index
    ds = rc.fixture_dataset(tmp_path, "train", num_rays=48, seed=3)
    assert ds.num_frames == 51 and len(ds) == 4 and list(ds.frames()) == [0, 1, 2, 3]
    assert [ds.sequence_index(k) for k in ds.frames()] == [1, 4, 7, 10]  # frame ids 4951, 4954, 4957, 4960 of 4950 ... 5000
    assert [ds.sequence_index(k) for k in ds.frames()] == [frame_index(ds.times[k], ds.num_frames) for k in ds.frames()]
    assert rc.fixture_dataset(tmp_path, "val", num_frames=11).num_frames == 11
    assert ds.scale == ds.scale and ds.fov == ds.fov_lidar and ds.num_rays == ds.num_rays_lidar == 48
    assert isinstance(ds.gen, torch.Generator) and not ds.device_batches
    # next_frame: every held frame once per epoch, in the order of the reference's loader (RandomSampler) for the torch seed
    torch.manual_seed(5)
    got = [ds.next_frame() for _ in range(12)]
    torch.manual_seed(5)
    want = [k for _ in range(3) for k in RandomSampler(range(4))]
    assert got == want and all(sorted(got[i:i + 4]) == [0, 1, 2, 3] for i in (0, 4, 8))
    # batch_for on the CPU == collate for the same generator state (collate draws from torch's global generator)
    for patch, n in ((1, 48), ([2, 8], 48)):
        ds.patch_size_lidar = patch
        ds.gen.manual_seed(7)
        x = ds.batch_for(2)
        torch.manual_seed(7)
        y = ds.collate([2])
        assert set(x) == set(y) | {"index", "time_host"} and x["index"] == [2]
        for k, v in y.items():
            assert (torch.equal(x[k], v) and x[k].dtype == v.dtype) if torch.is_tensor(v) else x[k] == v, k
        assert x["images_lidar"].dtype == torch.float16 and x["images_lidar"].shape == (1, n, 3)
        assert np.float32(x["time_host"]) == ds.times[2].numpy()[0] and frame_index(x["time_host"], 51) == 7
    ds.patch_size_lidar = 1
    torch.manual_seed(9)
    first = ds.next_frame()
    torch.manual_seed(9)
    ds2 = rc.fixture_dataset(tmp_path, "train", num_rays=48, seed=3)
    assert ds2.batch()["index"] == [first]
    # frame(k) == the non-training collate
    val = rc.fixture_dataset(tmp_path, "val")
    assert not val.training and val.num_rays_lidar == -1
    for k in val.frames():
        x, y = val.frame(k), val.collate([k])
        assert set(x) == set(y) | {"index", "time_host"}
        for name, v in y.items():
            assert torch.equal(x[name], v) if torch.is_tensor(v) else x[name] == v, name
        assert x["images_lidar"].shape == (1, 8, 32, 3)
    fr = ds.frame(1)  # a training split serves whole frames too (what the refine split is)
    assert fr["images_lidar"].shape == (1, 8, 32, 3) and fr["rays_d_lidar"].shape == (1, 256, 3)


def test_trainer_accepts_the_dataset(tmp_path, monkeypatch):
    """``Trainer(model, KITTI360Dataset(...))`` used to fail in the constructor with AttributeError (num_frames, images, poses)."""
    from lidar4d_amd import trainer as T
    ds = rc.fixture_dataset(tmp_path, "train")
    refine = rc.fixture_dataset(tmp_path, "refine")
    seen = []
    monkeypatch.setattr(T, "process_pointcloud", lambda d, removal=None: (seen.append(d), ({}, {}))[1])
    monkeypatch.setattr(T, "FlatAdam", lambda *a, **k: None)
    model = type("M", (), dict(_store=type("S", (), dict(flat=torch.zeros(1)))()))()
    tr = T.Trainer(model, ds, flow=True, loss_scaler=False, depth_loss="huber", raydrop_loss="bce", pointcloud_dataset=refine)
    assert tr.epoch_steps == 4 and seen == [refine] and tr.fused_losses  # ... whatever the criteria
    assert T.Trainer(model, ds, flow=True, loss_scaler=False).epoch_steps == 4 and seen[-1] is ds
    assert not T.Trainer(model, ds, flow=False, loss_scaler=False, fused_losses=False).fused_losses
    assert not tr.graphs_supported()  # a CPU dataset
    with pytest.raises(ValueError, match="unknown loss criterion"):
        T.Trainer(model, ds, flow=False, depth_loss="cos")


# ---- Trainer.train ------------------------------------------------------------------------------------------------------------------
def test_train_schedule(tmp_path, monkeypatch):
    """Three epochs over four frames: 12 steps in the dataset's permutation, patches in epoch 2 (change_patch_size_epoch = 2), the
    EMA updated after steps 4, 8 and 12, a checkpoint per epoch, an evaluation at the epochs eval_interval names, and the
    refinement on the refine split at the end."""
    from lidar4d_amd import checkpoint, trainer as T
    ds = rc.fixture_dataset(tmp_path, "train", num_rays=64)
    val, refine = rc.fixture_dataset(tmp_path, "val"), rc.fixture_dataset(tmp_path, "refine")
    tr = object.__new__(T.Trainer)
    steps, ema_at, saved, evaluated, refined, lines = [], [], [], [], [], []
    tr.dataset, tr.local_step, tr.epoch_steps, tr.iters = ds, 0, 4, 12
    tr.change_patch_size_lidar, tr.change_patch_size_epoch = [2, 8], 2
    tr.loss_kinds = dict(depth_loss="l1", raydrop_loss="bce", intensity_loss="mse")
    tr.model = type("M", (), dict(train=lambda self, mode=True: None, unet="unet"))()
    tr.opt = type("O", (), dict(lr=lambda self: 0.01))()
    tr.scaler = None
    tr.ema = type("E", (), dict(update=lambda self: ema_at.append(tr.local_step)))()

    def step(data):
        steps.append((data["index"][0], ds.patch_size_lidar, tuple(data["images_lidar"].shape)))
        return torch.tensor(float(len(steps)))

    tr._step_device_work = step
    tr.evaluate = lambda dataset, **kw: (evaluated.append((dataset, tr.local_step, kw)), {"loss": 0.5, "report": ["meter line"]})[1]
    tr.collect_refine_data = lambda dataset, **kw: (refined.append((dataset, tr.local_step)), ("inputs", "gts"))[1]
    monkeypatch.setattr(T, "refine_unet", lambda unet, x, gt, **kw: (refined.append((unet, x, gt, kw["epochs"])), [0.25])[1])
    monkeypatch.setattr(checkpoint, "save_checkpoint",
                        lambda path, model, opt, ema, scaler, **kw: saved.append((path, kw["epoch"], kw["global_step"], tr.local_step)))
    torch.manual_seed(5)
    hist = tr.train(valid_dataset=val, refine_dataset=refine, max_epochs=3, eval_interval=2, workspace=str(tmp_path / "ws"),
                    graphed=False, refine_iters=2, log=lines.append)
    torch.manual_seed(5)
    fresh = rc.fixture_dataset(tmp_path, "train")
    want_frames = [fresh.next_frame() for _ in range(12)]
    assert [s[0] for s in steps] == want_frames and len(steps) == 12 and tr.local_step == 12
    P = [2, 8]
    assert [s[1] for s in steps] == [1] * 4 + [P] * 4 + [1] * 4 and all(s[2] == (1, 64, 3) for s in steps)
    assert ema_at == [4, 8, 12]
    assert [(e, g, at) for _, e, g, at in saved] == [(1, 4, 4), (2, 8, 8), (3, 12, 12)]
    assert [p.split("/")[-2:] for p, *_ in saved] == [["checkpoints", f"lidar4d_ep{e:04d}.pth"] for e in (1, 2, 3)]
    assert [(d, at) for d, at, _ in evaluated] == [(val, 8)] and evaluated[0][2]["refine"] is False
    assert evaluated[0][2]["raydrop_loss"] == "bce"
    assert refined == [(refine, 12), ("unet", "inputs", "gts", 2)]
    assert hist["loss"] == [2.5, 6.5, 10.5] and [e for e, _ in hist["results"]] == [2] and hist["refine_loss"] == [0.25]
    assert any("Epoch 2" in l for l in lines) and "meter line" in lines
    # max_epochs defaults to ceil(iters / frames held); a second call continues after the epochs already made
    tr.iters = 18
    tr.train(graphed=False)
    assert len(steps) == 20 and tr.local_step == 20 and ema_at[-2:] == [16, 20]
