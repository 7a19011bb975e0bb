"""The fused line-of-sight loss (csrc/losses.hip, lidar4d_amd.trainer.line_of_sight_loss) on the device (``-m gpu``, MI355X):
against the reference's own train_step (tests/golden/train_step_losses.npz), against the torch restatement ``urf_loss`` it
replaces in the step, bit-for-bit against itself, with the tolerance read from the optimiser's device schedule, and inside a
Trainer: eager, and as part of a captured step.

Bounds.  Against the fixture: the rule of train_golden.check at rtol = 1e-4, what the fused primary-loss test uses against the
same file.  Against ``urf_loss``: 2e-5 relative on the value and 2e-5 of the largest magnitude on the gradient, the project's
figure for a fused node against its restatement; the two differ by fp32 rounding of single elements (a few
1e-7) and by the order of the sums (fp64 here, fp32 trees in torch: about 1e-6 at these sizes)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = 1000
STEPS = (0, 500, 1000, 2000)  # the last one is past iters: the exponent is clamped at 1
RTOL = 2e-5


def _eps(step, iters=ITERS):
    return 0.02 * 0.1 ** min(step / iters, 1)


def _random_case(N, T, seed, dropped=None, half=False):
    """Samples on a jittered ladder over (0.05, 1), depths in (0.2, 0.8), and around every depth a few samples inside the
    smallest tolerance (0.002), a few between the smallest and the largest (0.02), and -- on ray 0 -- one sample exactly on
    each bound of step 0, which is neither near nor empty."""
    g = torch.Generator().manual_seed(seed)
    d = 0.2 + 0.6 * torch.rand(N, generator=g)
    if dropped is not None:
        d[dropped] = 0.0
    if half:
        d = d.half()
    z = torch.linspace(0.05, 1.0, T).repeat(N, 1) + (torch.rand(N, T, generator=g) - 0.5) * (0.4 / T)
    offsets = (-0.0123, -0.0051, -0.0013, -0.0004, 0.0002, 0.0009, 0.0031, 0.0077, 0.0167)
    df = d.float()
    for j, off in enumerate(offsets[:max(T - 2, 0)]):
        z[:, (7 * j + 3) % T] = df + off
    if T >= 3:
        z[0, T - 1] = (d[0] - _eps(0)).float()  # torch's own `d - eps`: fp32, or rounded to half for a half depth
        z[0, T - 2] = (d[0] + _eps(0)).float()
    w = torch.rand(N, T, generator=g) * 0.3
    return w, z.float(), d


def _all_near_case():
    d = torch.tensor([0.30, 0.50, 0.70])
    off = torch.tensor([-0.015, -0.008, 0.004, 0.009, 0.016])
    z = d[:, None] + off[None, :]
    w = torch.linspace(0.15, 0.95, 15).reshape(3, 5).contiguous()
    return w, z, d


CASES = {
    "3x5_all_near": _all_near_case,
    "5x70_dropped_ray": lambda: _random_case(5, 70, 11, dropped=2),
    "1x1": lambda: (torch.tensor([[0.4]]), torch.tensor([[0.501]]), torch.tensor([0.5])),
    "67x200": lambda: _random_case(67, 200, 12),
    "5x70_half_depth": lambda: _random_case(5, 70, 13, half=True),
}
_cache = {}


def _case(name):
    if name not in _cache:
        _cache[name] = tuple(t.to(DEV) for t in CASES[name]())
    return _cache[name]


def _run(fn, w, z, d, step, scale=1.0, **kw):
    """-> (loss [0-dim], d loss * scale / d weights) of ``fn`` (urf_loss or line_of_sight_loss)."""
    leaf = w.clone().requires_grad_(True)
    loss = fn({"weights": leaf, "z_vals": z}, d.reshape(1, -1), step, ITERS, **kw)
    (loss * scale).backward()
    return loss.detach(), leaf.grad


def _reference(name, step, scale):
    from lidar4d_amd.trainer import urf_loss
    key = ("ref", name, step, scale)
    if key not in _cache:
        _cache[key] = _run(urf_loss, *_case(name), step, scale)
    return _cache[key]


# ---- 1. the reference's own train_step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["urf", "everything"])
def test_fused_term_vs_reference_train_step(tag, monkeypatch):
    """tests/golden/train_step_losses.npz (the loss block of the reference's Trainer.train_step): the total loss with the
    line-of-sight term from the fused node and every other term from the torch functions, and every gradient -- ``g_weights``
    comes from this term alone."""
    from lidar4d_amd import trainer as T
    from tests import train_golden
    c = train_golden.load(tag)
    assert bool(train_golden.opt_of(c)["urf_loss"]) and float(c["g_weights"].abs().max()) > 0.0
    entered = []

    def fused(out, gt_depth, step, iters):
        entered.append(step)
        return T.line_of_sight_loss(out, gt_depth, step, iters)

    monkeypatch.setattr(T, "urf_loss", fused)
    loss, leaves = train_golden.evaluate(c, device=DEV)
    assert entered == [int(c["global_step"])]
    train_golden.check(c, loss, leaves, rtol=1e-4)


# ---- 2. the torch restatement on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 512.0])
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("name", list(CASES))
def test_fused_term_vs_urf_loss(name, step, scale):
    from lidar4d_amd.trainer import line_of_sight_loss
    w, z, d = _case(name)
    want, g_want = _reference(name, step, scale)
    got, g_got = _run(line_of_sight_loss, w, z, d, step, scale)
    g_scale = float(g_want.abs().max())
    err_l = abs(float(got) - float(want)) / abs(float(want))
    err_g = float((g_got - g_want).abs().max()) / g_scale
    print(f"{name} step {step} x{scale:g}: loss {float(got):.9g} (torch {float(want):.9g}, rel {err_l:.2e}), gradient err / max = {err_g:.2e}")
    assert float(want) > 0.0 and g_scale > 0.0 and bool(torch.isfinite(g_got).all())
    assert err_l <= RTOL
    assert err_g <= RTOL
    assert g_got.shape == w.shape and g_got.dtype == torch.float32


def test_case_generator_makes_the_cases_it_is_meant_to():
    w, z, d = _case("67x200")
    for step in STEPS:
        e = _eps(step)
        near = (z > d[:, None] - e) & (z < d[:, None] + e)
        assert int(near.sum(1).min()) >= 2 and not bool(near.all())  # every ray has near samples; most samples are not near
    lo, hi = d[:, None] - _eps(0), d[:, None] + _eps(0)
    neither = ~((z > lo) & (z < hi)) & ~((z < lo) | (z > hi))
    assert int(neither[0].sum()) == 2 and int(neither.sum()) == 2  # the two samples planted on the bounds of step 0
    w, z, d = _case("5x70_half_depth")
    assert d.dtype == torch.float16
    lo, hi = d[:, None] - _eps(0), d[:, None] + _eps(0)
    assert lo.dtype == torch.float16 and int((~((z > lo) & (z < hi)) & ~((z < lo) | (z > hi))).sum()) == 2
    w, z, d = _case("5x70_dropped_ray")
    assert int((d > 0).sum()) == 4
    w, z, d = _case("3x5_all_near")
    assert bool(((z > d[:, None] - _eps(0)) & (z < d[:, None] + _eps(0))).all())


def test_normaliser_is_computed_not_assumed():
    """Every sample of the [3, 5] case lies within eps of its ray's depth at step 0, so the largest bell value is
    exp(-0.004^2 / (2 (0.02 / 3)^2)) = 0.835, not 1.  The loss with a normaliser of 1 is 0.0892 against 0.0971, 8 % off;
    the fused value has to be the true one, within the bound of the comparison above."""
    from lidar4d_amd.trainer import line_of_sight_loss
    w, z, d = _case("3x5_all_near")
    want, g_want = _reference("3x5_all_near", 0, 1.0)
    sigma = _eps(0) / 3.0
    bell = torch.exp(-((z - d[:, None]) ** 2) / (2 * sigma ** 2))
    assert abs(float(bell.max()) - math.exp(-0.004 ** 2 / (2 * sigma ** 2))) < 1e-5 and abs(float(bell.max()) - 0.835) < 1e-3
    assumed_one = 0.1 * float(((w - bell) ** 2).sum()) / 3
    true = 0.1 * float(((w - bell / bell.max()) ** 2).sum()) / 3
    assert abs(true - float(want)) <= 5e-6 * true
    assert abs(assumed_one - true) > 0.05 * true  # (far apart: 2500 times the bound below)
    got, g_got = _run(line_of_sight_loss, w, z, d, 0)
    print(f"all near: fused {float(got):.7f}, torch {float(want):.7f}, with a normaliser of 1 {assumed_one:.7f}")
    assert abs(float(got) - true) <= RTOL * true
    assert abs(float(got) - assumed_one) > 0.05 * true
    assert float((g_got - g_want).abs().max()) <= RTOL * float(g_want.abs().max())


# ---- 3. same bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["67x200", "5x70_half_depth", "3x5_all_near"])
def test_same_input_same_bits(name):
    from lidar4d_amd.trainer import line_of_sight_loss
    w, z, d = _case(name)
    a, ga = _run(line_of_sight_loss, w, z, d, 500, 512.0)
    torch.empty(1 << 20, device=DEV).fill_(float("nan"))  # (the workspace of the second call is not the first call's, nor clean)
    b, gb = _run(line_of_sight_loss, w, z, d, 500, 512.0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))


# ---- 4. the device schedule ---------------------------------------------------------------------------------------------------------
def test_tolerance_follows_the_device_schedule():
    from lidar4d_amd.trainer import line_of_sight_loss
    w, z, d = _case("67x200")
    at250, g250 = _run(line_of_sight_loss, w, z, d, 250)
    at750, g750 = _run(line_of_sight_loss, w, z, d, 750)
    assert float(at250) != float(at750)
    sched = torch.tensor([250.0, 1.0], device=DEV)
    got, g = _run(line_of_sight_loss, w, z, d, 987654, sched=sched)  # the global_step argument is not what counts
    assert torch.equal(got, at250) and torch.equal(g, g250)
    sched.add_(torch.tensor([500.0, 0.0], device=DEV))              # written on the device: the next call follows it
    got, g = _run(line_of_sight_loss, w, z, d, 250, sched=sched)
    assert torch.equal(got, at750) and torch.equal(g, g750)
    # forward and backward both read the schedule when they RUN: a backward after the optimiser's update would see the new count,
    # which is why the step evaluates loss and gradient before Adam
    leaf = w.clone().requires_grad_(True)
    loss = line_of_sight_loss({"weights": leaf, "z_vals": z}, d.reshape(1, -1), 0, ITERS, sched=sched)
    sched.add_(torch.tensor([-500.0, 0.0], device=DEV))
    loss.backward()
    assert torch.equal(loss.detach(), at750) and torch.equal(leaf.grad, g250)


# ---- 5. inside the Trainer ------------------------------------------------------------------------------------------------------------
def _small_trainer(**kw):
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.data import KITTI360_SCALE, SyntheticKitti360
    from lidar4d_amd.trainer import Trainer
    from oracle.detparams import fill_model
    from oracle.make_golden import SMALL_MODEL
    cfg = dict(SMALL_MODEL, num_frames=5, near_lidar=KITTI360_SCALE, far_lidar=81 * KITTI360_SCALE, density_scale=20.0)
    data = SyntheticKitti360(DEV, H=16, W=64, num_frames=5, num_rays=128)
    m = fill_model(LiDAR4D(**cfg), seed=3, flow_out_amp=0.002).to(DEV)
    return m, data, Trainer(m, data, num_steps=64, urf=True, chamfer=False, flow=False, init_scale=1.0, **kw)


def _loss_without_the_term(tr, batch, out):
    tr.urf = False
    try:
        return float(tr.compute_loss(batch, out))
    finally:
        tr.urf = True


def test_trainer_compute_loss_fused_vs_torch():
    """Trainer.compute_loss on the same render outputs with the fused node and with ``urf_loss``: value, and the gradient that
    reaches the render's ``weights``."""
    m, data, tr = _small_trainer(iters=10)
    assert tr.fused_urf and tr.graphs_supported()
    tr.opt.step_count = 3
    batch = data.batch_for(2)
    out = m.render(batch["rays_o_lidar"], batch["rays_d_lidar"], batch["time"], staged=False, perturb=False, num_steps=64,
                   time_host=batch.get("time_host"))
    res = {}
    for fused in (True, False):
        tr.fused_urf = fused
        loss = tr.compute_loss(batch, out)
        (g,) = torch.autograd.grad(loss, out["weights"], retain_graph=True)
        res[fused] = (float(loss), g)
    tr.fused_urf = False
    assert not tr.graphs_supported()  # the torch route computes the tolerance on the host
    (lf, gf), (lt, gt_) = res[True], res[False]
    plain = _loss_without_the_term(tr, batch, out)
    print(f"compute_loss: fused {lf:.8g}, torch {lt:.8g}; without the term {plain:.8g}")
    assert lt - plain > 1e-3 * lt, "the line-of-sight term is too small a part of this loss to be checked by it"
    assert abs(lf - lt) <= RTOL * abs(lt)
    assert float(gt_.abs().max()) > 0 and float((gf - gt_).abs().max()) <= RTOL * float(gt_.abs().max())


def test_captured_step_with_line_of_sight_term(monkeypatch):
    """``urf=True`` can be captured, and a REPLAY reproduces the eager step from the same state and batch (the scheme of
    test_graph_replay_equals_eager_step: static batch, no sample jitter, snapshot / restore), at three iteration counts: the
    tolerance inside the graph follows ``opt.sched[0]``, so the loss of the replay at count k is the eager loss at count k.
    Gradients within that test's 1e-3 of each tensor's largest value (the order of the dW atomics)."""
    from lidar4d_amd.params import bump_epoch
    m, data, tr = _small_trainer(iters=16, graph_batch_inside=False)
    assert tr.graphs_supported()
    st, opt = m._store, tr.opt
    batch = {k: (v.contiguous().clone() if torch.is_tensor(v) else v) for k, v in data.batch_for(2).items()}
    monkeypatch.setattr(data, "batch_for", lambda frame: batch)
    render = m.render
    monkeypatch.setattr(m, "render", lambda *a, **kw: render(*a, **{**kw, "perturb": False}))
    for _ in range(3):
        tr.train_step(batch)
    opt.device_schedule()
    assert opt.sched.tolist()[0] == 3.0 == float(opt.step_count)
    snap = {"flat": st.flat.detach().clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(), "steps": opt.steps.clone(),
            "scaler": tr.scaler.state.clone(), "sched": opt.sched.clone(), "count": opt.step_count}

    def restore(k=0):
        """the snapshot's parameters and optimiser state, at iteration count snapshot + k"""
        with torch.no_grad():
            st.flat.copy_(snap["flat"]), opt.exp_avg.copy_(snap["m"]), opt.exp_avg_sq.copy_(snap["v"]), opt.steps.copy_(snap["steps"])
            tr.scaler.state.copy_(snap["scaler"]), opt.sched.copy_(snap["sched"])
            opt.sched[0] += float(k)
        opt.step_count = snap["count"] + k
        bump_epoch()
        st.refresh16()

    counts = (0, 2, 5)
    eager = {}
    for k in counts:
        restore(k)
        loss = float(tr.train_step(batch))
        eager[k] = (loss, st.flat_grad.detach().clone())
        assert np.isfinite(loss) and bool(torch.isfinite(eager[k][1]).all()) and not torch.equal(st.flat, snap["flat"])
    assert len({eager[k][0] for k in counts}) == len(counts), "the loss does not move with the iteration count"
    restore(0)
    tr.train_step_graphed(2)  # eager warm-up + capture
    for k in counts:
        restore(k)
        loss = float(tr.train_step_graphed(2))
        l_e, g_e = eager[k]
        print(f"count +{k}: replay loss {loss:.8g}, eager {l_e:.8g}")
        assert abs(loss - l_e) <= RTOL * abs(l_e), f"replay at count +{k}: loss {loss} against the eager step's {l_e}"
        for name, p, off, n, gi in st.entries:
            if not n:
                continue
            a, b = st.flat_grad[off:off + n], g_e[off:off + n]
            assert bool(torch.isfinite(a).all()), f"replay at count +{k}: non-finite gradient in {name}"
            d = float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)
            assert d < 1e-3, f"replay at count +{k}: gradient of {name} differs from the eager step's by {d:.2e} of its largest value"
    # the replay at the WRONG count is not the eager step at the right one (so the comparison above can tell)
    spread = min(abs(eager[a][0] - eager[b][0]) for a in counts for b in counts if a < b)
    assert spread > 10 * RTOL * abs(eager[0][0])
    # ... and consecutive replays advance the schedule themselves
    restore(0)
    for _ in range(3):
        tr.train_step_graphed(2)
    assert opt.sched.tolist()[0] == snap["sched"].tolist()[0] + 3 and opt.step_count == snap["count"] + 3
    assert len(tr._step_graphs["graphs"]) == 1
