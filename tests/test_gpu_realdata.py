"""Training on a preprocessed sequence, on the device (``-m gpu``, MI355X): the sixth library's two entry points
(include/lidar4d_step.h) against the torch route and against an exact numpy emulation of the default criteria, the fused
primary-loss node on both train-step fixtures, and ``Trainer`` on ``KITTI360Dataset`` with fp16 ground truth -- eager, captured,
and as the reference's whole ``train()``."""
import itertools

import numpy as np
import pytest
import torch

import realdata_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("l1", "mse", "bce", "huber")


# ---- l4ds_ray_batch -----------------------------------------------------------------------------------------------------------------
def _torch_batch(ds, k, top, left, px, py):
    """The torch route for given corners: data.get_lidar_rays' expansion (patch-row major, columns wrapping), its per-pixel ray
    formulas (taken from the whole frame's rays) and the gather of kitti360_dataset.py:181-187."""
    from lidar4d_amd.data import get_lidar_rays
    W = ds.W_lidar
    dr = torch.arange(px, device=DEV).repeat_interleave(py)
    dc = torch.arange(py, device=DEV).repeat(px)
    inds = ((top[:, None] + dr[None, :]).reshape(-1) * W + ((left[:, None] + dc[None, :]) % W).reshape(-1))
    rays = get_lidar_rays(ds.poses_lidar[k:k + 1], ds.intrinsics_lidar, ds.H_lidar, W, -1)
    return inds[None], rays["rays_o"][:, inds], rays["rays_d"][:, inds], ds.images_lidar[k].reshape(-1, 3)[inds][None]


@pytest.mark.parametrize("fp16", [True, False])
def test_ray_batch_equals_torch_route(tmp_path, fp16):
    """ops.ray_batch_patches against the torch route for the same corners: single pixels at n = 1, 255, 256, 257 (one workgroup
    short of, at, and past its 256 threads) and 2 x 8 patches whose left corners sit in the last columns (the wrap at W): the same
    ``inds``, bit-equal ground truth IN THE FRAME'S DTYPE, bit-equal origins, directions within 2e-7 (the bound of
    test_fused_ray_batch_equals_get_lidar_rays: the torch path rotates with a batched GEMM); twice the same bits."""
    from lidar4d_amd import ops
    ds = rc.fixture_dataset(tmp_path, "train", device=DEV, fp16=fp16)
    H, W, dt = ds.H_lidar, ds.W_lidar, torch.float16 if fp16 else torch.float32
    assert ds.images_lidar.dtype == dt and ds.images_lidar.is_cuda
    g = torch.Generator(device=DEV).manual_seed(1)
    draws = [(1, 1, torch.randint(0, H - 1, [n], device=DEV, generator=g), torch.randint(0, W, [n], device=DEV, generator=g))
             for n in (1, 255, 256, 257)]
    draws.append((2, 8, torch.randint(0, H - 2, [17], device=DEV, generator=g), torch.randint(W - 9, W, [17], device=DEV, generator=g)))
    draws.append((2, 8, torch.tensor([H - 2, 0], device=DEV), torch.tensor([W - 1, W - 8], device=DEV)))
    for k, (px, py, top, left) in zip(itertools.cycle(range(4)), draws):
        args = (top, left, (px, py), ds.poses_lidar[k], ds.intrinsics_lidar, H, W, ds.images_lidar[k])
        rays_o, rays_d, gt, inds = ops.ray_batch_patches(*args)
        w_inds, w_o, w_d, w_gt = _torch_batch(ds, k, top, left, px, py)
        n = top.numel() * px * py
        assert inds.shape == (1, n) and gt.shape == (1, n, 3) and gt.dtype == dt and rays_d.dtype == torch.float32
        assert torch.equal(inds, w_inds) and torch.equal(gt, w_gt) and torch.equal(rays_o, w_o)
        assert float((rays_d - w_d).abs().max()) <= 2e-7
        if py > 1:
            assert int((inds % W).max()) == W - 1 and int((inds % W).min()) == 0  # both sides of the wrap
        again = ops.ray_batch_patches(*args)
        assert all(torch.equal(a, b) for a, b in zip((rays_o, rays_d, gt, inds), again))
        no_gt = ops.ray_batch_patches(*args[:-1])
        assert no_gt[2] is None and torch.equal(no_gt[1], rays_d)


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("patch,n", [(1, 255), (1, 256), ([2, 8], 256), ([2, 8], 16), (1, 1)])
def test_batch_for_equals_torch_route(tmp_path, fp16, patch, n):
    """KITTI360Dataset.batch_for on the device (two randints + one launch) against its own torch route (get_lidar_rays + gather)
    for the same generator state; the generator is left in the same state."""
    a = rc.fixture_dataset(tmp_path, "train", device=DEV, fp16=fp16, num_rays=n, seed=9, patch_size_lidar=patch)
    b = rc.fixture_dataset(tmp_path, "train", device=DEV, fp16=fp16, num_rays=n, seed=9, patch_size_lidar=patch)
    b.preload = False  # (its tensors stay where they are: only the route changes)
    assert a.device_batches and not b.device_batches
    for k in (2, 0, 2):
        x, y = a.batch_for(k), b.batch_for(k)
        assert set(x) == set(y)
        for name in ("rays_o_lidar", "rays_d_lidar", "images_lidar", "time", "poses_lidar"):
            assert x[name].shape == y[name].shape and x[name].dtype == y[name].dtype, name
        assert x["images_lidar"].dtype == (torch.float16 if fp16 else torch.float32) and x["images_lidar"].shape == (1, n, 3)
        assert torch.equal(x["images_lidar"], y["images_lidar"]) and torch.equal(x["rays_o_lidar"], y["rays_o_lidar"])
        assert float((x["rays_d_lidar"] - y["rays_d_lidar"]).abs().max()) <= 2e-7
        assert torch.equal(x["time"], y["time"]) and x["time_host"] == y["time_host"] and x["index"] == y["index"] == [k]
    assert torch.equal(torch.randint(0, 1000, [8], device=DEV, generator=a.gen), torch.randint(0, 1000, [8], device=DEV, generator=b.gen))


# ---- l4ds_primary_losses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,tag", rc.ALL_CASES)
def test_fused_losses_vs_reference_train_step(which, tag):
    """Every case of both train-step fixtures (the reference's own train_step on fp32 and on fp16 ground truth) with the primary
    losses + ray chamfer, the line-of-sight term and the patch terms on their fused nodes: loss and every gradient at 1e-4, the
    device bound of tests/test_gpu_glue.py."""
    c = rc.load(which, tag)
    loss, leaves = rc.evaluate_fused(c, DEV)
    rc.train_golden.check(c, loss, leaves, rtol=1e-4)


def _loss_inputs(n, half, seed=0):
    return rc.loss_inputs(n, half, seed, DEV)


@pytest.mark.parametrize("n", rc.PRIMARY_REF_N)
def test_default_criteria_on_fp32_equal_lidar_losses_bit_for_bit(n):
    """l1 / mse / mse on fp32 ground truth: l4ds_primary_losses gives the bits of rc.primary_losses_ref, the numpy float32
    evaluation in the kernel's order that no HIP code computes (tests/test_realdata_cpu.py pins it against float64): loss through
    the fixed-order sum of csrc/glue_dev.h, both gradients, both point sets and the fp32 copy of the ground truth.  n on both
    sides of a workgroup, and 65,793 rays = 258 partials, where the second stage's strided loop takes a second turn."""
    from lidar4d_amd import ops
    depth, image, gt, rays_d, S = _loss_inputs(n, half=False, seed=n)
    host = [t.cpu().numpy() for t in (depth, image, gt, rays_d)]
    for smooth, alphas in rc.PRIMARY_REF_SETTINGS:
        want = {k: torch.from_numpy(v) for k, v in rc.primary_losses_ref(*host, *alphas, smooth, S).items()}
        for points in (True, False):
            new = ops.primary_losses_any(depth, image, gt, rays_d, ("l1", "mse", "mse"), *alphas, smooth, 0.2 * S, S, want_points=points,
                                         want_gt32=True)
            got = dict(zip(("loss", "g_depth", "g_image", "pts", "gt32"), new))
            assert float(got["loss"]) != 0.0
            if not points:
                assert got.pop("pts") is None
            for name, t in got.items():
                assert torch.equal(t.cpu(), want[name]), (name, points, smooth)


@pytest.mark.parametrize("half", [True, False])
def test_entry_points_give_the_same_bits_twice(half):
    from lidar4d_amd import ops
    depth, image, gt, rays_d, S = _loss_inputs(1000, half=half, seed=3)
    for kinds in (("l1", "mse", "mse"), ("huber", "bce", "l1"), ("bce", "huber", "huber")):
        runs = [ops.primary_losses_any(depth, image, gt, rays_d, kinds, 1.0, 0.01, 0.1, 0.2, 0.2 * S, S, want_points=True, want_gt32=half)
                for _ in range(2)]
        for a, b in zip(*runs):
            assert (a is None and b is None) or torch.equal(a, b)
        assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][1].abs().max()) > 0
        if half:
            assert torch.equal(runs[0][4], gt.float())


def test_no_rays_write_a_zero_loss_and_nothing_else():
    """n == 0: loss_out[0] = 0; sentinels on either side of every output stay what they were."""
    from lidar4d_amd import _step_lib, ops
    buf = torch.full((64,), 7.5, dtype=torch.float32, device=DEV)
    at = lambda i: ops._p(buf[i:])
    ws = torch.full((4,), 7.5, dtype=torch.float32, device=DEV)
    assert _step_lib.lib().l4ds_primary_losses_workspace(0) == 4
    # loss at [8]; the empty outputs g_depth, g_image, pts, gt32 at [16], [24], [32], [40]: every neighbour is a sentinel
    _step_lib.call("l4ds_primary_losses", None, None, None, 1, None, 0, 3, 2, 0, 1.0, 0.01, 0.1, 0.2, 0.002, 0.01, at(8), at(16), at(24),
                   at(32), at(40), ops._p(ws[1:]), ops._stream())
    torch.cuda.synchronize()
    want = torch.full((64,), 7.5)
    want[8] = 0.0
    assert torch.equal(buf.cpu(), want)
    assert float(ws[0]) == 7.5 and float(ws[2]) == 7.5 and float(ws[3]) == 7.5  # (ws[1]: the workspace's one partial, free to change)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    out = ops.primary_losses_any(z(0), z(0, 2), z(0, 3, dt=torch.float16), z(0, 3), ("huber", "bce", "l1"), 1.0, 0.01, 0.1, 0.2, 0.002, 0.01,
                                 want_points=True, want_gt32=True)
    assert float(out[0]) == 0.0 and out[1].shape == (0,) and out[3].shape == (2, 0, 3)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    rays = ops.ray_batch_patches(empty, empty, (2, 8), torch.eye(4, device=DEV), (2.0, 26.9), 8, 32, z(8, 32, 3))
    assert rays[0].shape == (1, 0, 3) and rays[3].shape == (1, 0)


@pytest.mark.parametrize("depth_loss,raydrop_loss", list(itertools.product(KINDS, KINDS)))
def test_every_criterion_pair_equals_lidar_loss(depth_loss, raydrop_loss):
    """All 16 depth x ray-drop criteria (intensity mse) at 257 rays, fp16 and fp32 ground truth: the fused node against
    ``lidar_loss`` on the device, loss and both gradients at 1e-4 (tests/train_golden.py's measure), under an upstream gradient
    that is not 1."""
    from lidar4d_amd.trainer import lidar_loss, primary_losses
    for half in (True, False):
        depth0, image0, gt, rays_d, S = _loss_inputs(257, half=half, seed=11)
        res = {}
        for name in ("torch", "fused"):
            depth, image = depth0[None].clone().requires_grad_(True), image0[None].clone().requires_grad_(True)
            out, kinds = {"depth_lidar": depth, "image_lidar": image}, dict(depth_loss=depth_loss, raydrop_loss=raydrop_loss)
            if name == "torch":
                loss = lidar_loss(out, gt[None], scale=S, **kinds)
            else:
                loss = primary_losses(out, {"images_lidar": gt[None], "rays_d_lidar": rays_d[None]}, S, chamfer=False, **kinds)
            (loss * 16.0).backward()
            res[name] = (float(loss.detach()), depth.grad, image.grad)
        (lt, dt_, it_), (lf, df, if_) = res["torch"], res["fused"]
        print(f"{depth_loss}/{raydrop_loss} half={half}: loss {lf} vs {lt}")
        assert np.isfinite(lt) and abs(lf - lt) <= 1e-4 * max(1.0, abs(lt)), (half, lf, lt)
        for got, want, what in ((df, dt_, "d/d depth"), (if_, it_, "d/d image")):
            scale = float(want.abs().max())
            assert scale > 0 and float((got - want).abs().max()) <= 1e-4 * scale + 1e-9, (half, what, float((got - want).abs().max()), scale)


# ---- a training step on the fixture sequence ------------------------------------------------------------------------------------------
def _small_model(seed=11, **kw):
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE
    from oracle.detparams import fill_model
    from oracle.make_golden import SMALL_MODEL
    cfg = dict(SMALL_MODEL, density_scale=20.0, near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE, **kw)
    return fill_model(LiDAR4D(**cfg), seed=seed).to(DEV)


def _trainer(tmp_path, num_rays=64, H=8, W=32, **kw):
    from lidar4d_amd.trainer import Trainer
    data = rc.fixture_dataset(tmp_path, "train", device=DEV, num_rays=num_rays, seed=3, H=H, W=W)
    refine = rc.fixture_dataset(tmp_path, "refine", device=DEV, H=H, W=W)
    assert data.images_lidar.dtype == torch.float16
    kw = dict(dict(num_steps=64, iters=100, chamfer=True, flow=True, init_scale=1.0, point_removal=rc.split_on_z(-1.0),
                   pointcloud_dataset=refine), **kw)
    return Trainer(_small_model(), data, **kw), data


@pytest.mark.parametrize("kinds", [("l1", "mse", "mse"), ("huber", "bce", "l1"), ("mse", "l1", "huber")])
def test_trainer_step_fused_equals_torch_losses_on_fp16_ground_truth(tmp_path, kinds):
    """``Trainer(model, KITTI360Dataset(...))`` -- an AttributeError in the constructor before.  One step from the same state,
    batch and seeds with the fused nodes and with the torch restatement, three criterion sets: the losses within 1e-4, the bound
    of test_trainer_step_fused_equals_torch_losses, and the gradient arenas (read before the optimiser touches them) within 5e-3
    in relative L2, the bound tests/test_gpu_glue.py::test_fused_flow_loss_equals_torch_path sets for the loosest part of the
    fused step: the scene-flow node's fp16 adjoints, 2^-11 per rounding and a handful of roundings down the chain.
    (That test's count of parameters which Adam moved differently is not asserted here: with 64 rays on an 8 x 32 frame a few
    thousand table entries have gradients that cancel to 1e-8 of their table's largest, Adam's first step turns their sign or
    zero-ness into a full +-lr, and the count -- 2.6e-3 with fp16 and 3.0e-3 with fp32 ground truth, measured, none of it
    without the ray-chamfer term -- says nothing about the losses under test.)"""
    outs = {}
    for fused in (True, False):
        tr, data = _trainer(tmp_path, fused_losses=fused, depth_loss=kinds[0], raydrop_loss=kinds[1], intensity_loss=kinds[2])
        assert tr.fused_losses == fused and sorted(tr.pc_list) == ["1", "10", "4", "7"]
        start = tr.model._store.flat.detach().clone()
        data.gen.manual_seed(21)
        batch = data.batch_for(2)
        assert batch["images_lidar"].dtype == torch.float16
        grads, step = [], tr.opt.step
        tr.opt.step = lambda **kw: (grads.append(tr.model._store.flat_grad.detach().clone()), step(**kw))[1]
        torch.manual_seed(5)  # (perturbation noise and the ground-point time of the scene-flow loss)
        outs[fused] = (float(tr.train_step(batch).detach()), grads[0])
        assert float((tr.model._store.flat.detach() - start).abs().max()) > 0
    (la, ga), (lb, gb) = outs[True], outs[False]
    rel = float((ga - gb).norm() / gb.norm())
    print(f"{kinds}: fused {la}, torch {lb}; gradient arenas differ by {rel:.2e} in relative L2")
    assert np.isfinite(la) and abs(la - lb) <= 1e-4 * abs(lb), (la, lb)
    assert bool(torch.isfinite(ga).all()) and float(gb.norm()) > 0 and rel <= 5e-3, rel


def test_half_ground_truth_reaches_the_fused_nodes_as_half(tmp_path, monkeypatch):
    """urf=True in a patch step: the line-of-sight node and the patch node receive the fp16 batch as half (they were built for it),
    the primary-loss node too."""
    from lidar4d_amd import ops, trainer as T
    seen = {}

    def spy(name, fn, pick):
        def wrapped(*a, **k):
            seen[name] = [t.dtype for t in pick(a)]
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(T, "line_of_sight_loss", spy("los", T.line_of_sight_loss, lambda a: [a[1]]))
    monkeypatch.setattr(T, "patch_depth_grad_loss", spy("patch", T.patch_depth_grad_loss, lambda a: [a[1], a[2]]))
    monkeypatch.setattr(ops, "primary_losses_any", spy("primary", ops.primary_losses_any, lambda a: [a[2]]))
    tr, data = _trainer(tmp_path, urf=True)
    data.patch_size_lidar = [2, 8]
    loss = float(tr.train_step().detach())
    assert np.isfinite(loss)
    assert seen == {"los": [torch.float16], "patch": [torch.float16] * 2, "primary": [torch.float16]}


def test_captured_steps_over_an_epoch(tmp_path):
    """A preloaded KITTI360Dataset on the device supports captured steps.  Two epochs of train_step_graphed -- every frame's graph
    captured, then replayed -- against as many eager steps of a second trainer: what tests/test_gpu_optim.py compares for a
    captured step that draws its own batch (gradients finite, parameters move, counters), and the loss scale and step counts
    advance as in the eager steps."""
    tr, data = _trainer(tmp_path)  # (loss scale 1, as in the other steps on the small model: nothing overflows, no step is skipped)
    eager, _ = _trainer(tmp_path)
    assert tr.graphs_supported() and data.device_batches
    torch.manual_seed(5)
    losses, frames = [], []
    for it in range(8):
        before = tr.model._store.flat.clone()
        frame = data.next_frame()
        frames.append(frame)
        losses.append(float(tr.train_step_graphed(frame)))
        assert np.isfinite(losses[-1]) and bool(torch.isfinite(tr.model._store.flat_grad).all()), it
        assert not torch.equal(tr.model._store.flat, before), f"step {it} did not move the parameters"
    assert sorted(frames[:4]) == sorted(frames[4:]) == [0, 1, 2, 3] and len(tr._step_graphs["graphs"]) == 4
    for frame in frames:
        eager.train_step(eager.dataset.batch_for(frame))
    torch.cuda.synchronize()
    assert tr.opt.step_count == eager.opt.step_count == 8 and tr.local_step == eager.local_step == 8
    assert tr.opt.sched.tolist()[0] == 8.0 and abs(tr.opt.sched.tolist()[1] - 0.1 ** (7 / 100)) < 1e-6
    assert tr.scaler.state_dict() == eager.scaler.state_dict() and tr.scaler.state_dict()["_growth_tracker"] == 8
    assert torch.equal(tr.opt.steps, eager.opt.steps)


def test_train_runs_the_reference_schedule(tmp_path):
    """Trainer.train on the fixture sequence (16 x 64 here: the U-Net halves the image four times) with fp16 ground truth: two
    epochs, patches in the second, the EMA, validation on ``val``, a checkpoint per epoch, the refinement on ``refine``.  The
    checkpoint then loads into a fresh trainer, and a step made there is bit-equal in its loss to the step the first trainer
    makes next under equal generator states -- both on the EMA weights the refinement leaves in place (runner.py:819-821).  The
    loss is what can be compared bit for bit: it is computed before the backward, whose gradient scatter adds with float atomics."""
    from lidar4d_amd.checkpoint import latest_checkpoint
    size = dict(H=16, W=64)
    tr, data = _trainer(tmp_path, ema_decay=0.95, change_patch_size_lidar=[2, 8], **size)
    val = rc.fixture_dataset(tmp_path, "val", device=DEV, **size)
    refine = rc.fixture_dataset(tmp_path, "refine", device=DEV, **size)
    lines = []
    torch.manual_seed(5)
    hist = tr.train(valid_dataset=val, refine_dataset=refine, max_epochs=2, eval_interval=1, workspace=str(tmp_path / "ws"),
                    refine_iters=2, log=lines.append)
    assert len(hist["loss"]) == 2 and all(np.isfinite(v) for v in hist["loss"]) and len(hist["refine_loss"]) == 2
    assert [e for e, _ in hist["results"]] == [1, 2] and tr.local_step == 8 and tr.ema.num_updates == 2
    assert sorted(tr._step_graphs["graphs"], key=str) == sorted([(k, p) for k in range(4) for p in (1, (2, 8))], key=str)  # (held frame, patch)
    for _, res in hist["results"]:
        assert np.isfinite(res["loss"]) and len(res["report"]) == 4
        for meter in ("raydrop", "intensity", "depth", "points"):
            assert res[meter] is not None and len(np.atleast_1d(np.asarray(res[meter], dtype=np.float64))) >= 1, meter
    path = latest_checkpoint(str(tmp_path / "ws" / "checkpoints"), "lidar4d")
    assert path.endswith("lidar4d_ep0002.pth")
    fresh, data2 = _trainer(tmp_path, ema_decay=0.95, change_patch_size_lidar=[2, 8], **size)
    info = fresh.load(path)
    assert info["global_step"] == 8 == fresh.local_step and info["epoch"] == 2 and fresh.opt.step_count == tr.opt.step_count == 8
    assert fresh.scaler.state_dict() == tr.scaler.state_dict() and fresh.ema.num_updates == 2
    fresh.ema.copy_to()  # (the first trainer's refinement did the same)
    assert torch.equal(fresh.model._store.flat, tr.model._store.flat) and torch.equal(fresh.opt.exp_avg, tr.opt.exp_avg)
    got = []
    for t, d in ((tr, data), (fresh, data2)):
        t.model.train()
        d.patch_size_lidar = 1  # epoch 3 draws single pixels again (train_step sets it, but this batch is drawn before)
        d.gen.manual_seed(33)
        torch.manual_seed(7)
        got.append(t.train_step(d.batch_for(1)).detach().clone())
        assert t.dataset.patch_size_lidar == 1 and t.local_step == 9
    assert torch.equal(got[0], got[1]) and bool(torch.isfinite(got[0]))
