"""The loss kernels on the routes their feature tests do not enter (``-m gpu``, MI355X): csrc/losses.hip (line-of-sight loss) and
csrc/stepglue.hip (primary losses, ray batch) against the references of tests/loss_ref.py, which no HIP code computes and which
tests/test_loss_ref_cpu.py pins against the float64 restatements.  The table in tests/loss_ref.py's docstring names the loop or
branch each case enters.  The largest tensor here is [8197, 8].

Bounds, and where each comes from.

Line-of-sight loss against los_ref64: the loss within 1e-6 relative, the gradient within 1e-6 of its largest magnitude.  A term
w - bell / m is formed by at most about eight fp32 roundings of 2^-24 = 6e-8 each (x, x * x, the quotient, expf at <= 2 ulp, / m,
the subtraction, coef, the product): 5e-7, doubled.  The sums are fp64 on both sides.  The float32 restatement on the CPU sits at
1.5e-7 on the same cases (test_los_ref64_vs_urf_loss_in_float32 prints it and demands 5e-7).  With no ray that has a return the
reference's IEEE result is demanded instead: NaN for NaN, inf for inf of the same sign.  A wrong normaliser moves the loss of the
three cases built for it by more than 1e-3 relative (asserted on the CPU), a thousand times the bound.

The C entry points with pointers that are not 16-byte aligned (the scalar route at T % 4 == 0): the gradient has the BITS of the
aligned call -- it is element-wise behind a max and an integer count.  The loss is the fp32 rounding of fp64 sums whose per-lane
order differs between the two routes (a lane adds samples 4 lane .. 4 lane + 3 of each 256 on one and sample lane of each 64 on
the other), so its bits are not promised; they were equal on every case here when this was written and the test demands it, since
the inputs are fixed: should that ever change with the compiler, the 1e-6 bound above is the one that applies.

Primary losses without BCE: every output has the bits of primary_losses_emul, the numpy float32 evaluation in the kernel's order.
With BCE somewhere: the outputs no exp or log1p feeds (points, the fp32 copy of the ground truth, the gradient columns of the
BCE-free terms) are still bit-equal; the others are compared with primary_losses_ref64 (float64), per element within
4 x loss_ref.BCE_DEVIATION x 2^-24 of that output's largest magnitude.  BCE_DEVIATION is what the emulation itself -- numpy's
float32 exp and log1p -- deviates from the float64 reference on the same inputs, measured on the CPU by
tests/test_loss_ref_cpu.py::test_emulation_against_float64: 3.16 (loss), 2.58 (g_depth) and 8.47 (g_image) units of 2^-24,
stated as 3.2, 2.6 and 8.5; the bounds are therefore 12.8, 10.4 and 34 units, 7.6e-7, 6.2e-7 and 2.0e-6 of the largest magnitude.
The factor 4 allows the device's expf / log1pf to differ from numpy's by an ulp or two.  At saturating logits everything is
finite and the saturated values are exact.

Ray batch against ray_batch_ref64: indices, ground truth (zeros for a row outside [0, H), which include/lidar4d_step.h promises)
and origins equal; directions within 2e-7 of the float64 evaluation of the formulas, the bound of
test_ray_batch_equals_torch_route.  1.85e-7 was measured on the MI355X, of which the kernel's float32 pi accounts for a part: against
the same formulas with that pi the deviation is 1.5e-7 (both are printed)."""
import numpy as np
import pytest
import torch

import loss_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOS_TOL = 1e-6
UPSTREAM = (1.0, 512.0)
F16, F32, F64 = np.float16, np.float32, np.float64
_cache = {}


# ---- line-of-sight loss -------------------------------------------------------------------------------------------------------------
def _dev(name):
    if name not in _cache:
        _cache[name] = tuple(t.to(DEV) for t in L.los_case(name))
    return _cache[name]


def _run(w, z, d, step, scale=1.0):
    """-> (loss float, d (loss * scale) / d weights as numpy) of trainer.line_of_sight_loss."""
    from lidar4d_amd.trainer import line_of_sight_loss
    leaf = w.clone().requires_grad_(True)
    loss = line_of_sight_loss({"weights": leaf, "z_vals": z}, d.reshape(1, -1), step, L.ITERS)
    (loss * scale).backward()
    assert leaf.grad.shape == w.shape and leaf.grad.dtype == torch.float32
    return loss.detach(), leaf.grad


@pytest.mark.parametrize("scale", UPSTREAM)
@pytest.mark.parametrize("step", L.STEPS)
@pytest.mark.parametrize("name", list(L.LOS_CASES))
def test_line_of_sight_loss_vs_float64(name, step, scale):
    want, g_want = L.los_reference(name, step, scale)
    got, g_got = _run(*_dev(name), step, scale)
    got, g_got = float(got), g_got.cpu().numpy()
    if name == "4x8_all_dropped":
        assert not np.isfinite(want) and not np.isfinite(g_want).any()
        assert L.same_pattern(got, want) and L.same_pattern(g_got, g_want), (got, want, g_got, g_want)
        return
    g_top = float(np.abs(g_want).max())
    err_l, err_g = abs(got - want) / want, float(np.abs(g_got - g_want).max()) / g_top
    print(f"{name} step {step} x{scale:g}: loss {got:.9g} (float64 {want:.9g}, rel {err_l:.2e}), gradient err / max = {err_g:.2e}")
    assert want > 0 and g_top > 0 and np.isfinite(g_got).all()
    assert err_l <= LOS_TOL
    assert err_g <= LOS_TOL


@pytest.mark.parametrize("name", list(L.LOS_FIRST_CHUNKS))
def test_normaliser_comes_from_the_whole_row(name):
    """3x260: the first 256 samples of every ray are near and the last four are not, so the normaliser is exactly 1 -- a pre-pass
    that stopped after its first chunk would have found 0.49.  3x520 and 3x130: every sample is near and the one closest to the
    depth sits in the third chunk, so the normaliser is 0.835 -- one that stopped early would have found 0.49, one that assumed a
    sample that is not near would have used 1.  The fused loss is the reference's with the true normaliser and more than 1e-3
    away from either wrong one."""
    w, z, d = L.los_case(name)
    true, _ = L.los_reference(name, 0)
    early, _ = L.los_reference(name, 0, m=L.los_bell_max(z.numpy(), d.numpy(), 0, L.LOS_FIRST_CHUNKS[name]))
    one, _ = L.los_reference(name, 0, m=1.0)
    got = float(_run(*_dev(name), 0)[0])
    print(f"{name}: fused {got:.9g}, float64 {true:.9g}; first chunks only {early:.9g}, normaliser 1 {one:.9g}")
    assert abs(got - true) <= LOS_TOL * true
    assert abs(got - early) > 1e-3 * true
    if name == "3x260_near_then_far":
        assert one == true
    else:
        assert abs(got - one) > 1e-3 * true


def _los_call(name, which, step, offsets):
    """l4dl_los_fwd (``which`` = "fwd") or l4dl_los_bwd on the case's tensors placed inside larger buffers, ``offsets`` floats past
    the (16-byte aligned) start of the buffer for weights, z_vals and d_weights -> (result, the d_weights buffer, its data slice)."""
    from lidar4d_amd import _loss_lib, ops
    w, z, d = _dev(name)
    N, T = z.shape
    n = N * T

    def place(t, off, fill):
        buf = torch.full((n + 8,), fill, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        if t is not None:
            buf[off:off + n] = t.reshape(-1)
        return buf

    bw, bz, bd = place(w, offsets[0], 0.25), place(z, offsets[1], 0.5), place(None, offsets[2], 7.5)
    ws = torch.full((int(_loss_lib.lib().l4dl_los_workspace(N, T)),), 0xFF, dtype=torch.uint8, device=DEV)
    args = (ops._p(bw[offsets[0]:]), ops._p(bz[offsets[1]:]), ops._p(d), 0, N, T, None, step, L.ITERS)
    if which == "fwd":
        loss = torch.full((3,), 7.5, dtype=torch.float32, device=DEV)
        _loss_lib.call("l4dl_los_fwd", *args, ops._p(loss[1:]), ops._p(ws), ops._stream())
        assert float(loss[0]) == 7.5 and float(loss[2]) == 7.5
        return loss[1:2].clone(), None, None
    g = torch.tensor([512.0], device=DEV)
    _loss_lib.call("l4dl_los_bwd", *args, ops._p(g), ops._p(bd[offsets[2]:]), ops._p(ws), ops._stream())
    return None, bd, slice(offsets[2], offsets[2] + n)


@pytest.mark.parametrize("name", ["40x768", "8197x8"])
def test_c_entry_points_with_unaligned_pointers(name):
    """T % 4 == 0 with weights, z_vals or (backward) d_weights one float past a 16-byte boundary -- all three, and each alone --
    takes the scalar kernels: the result has the bits of the aligned call (see the module docstring for why the loss's are demanded
    although only the gradient's are promised), agrees with the float64 reference, and the floats on either side of the
    d_weights that was written keep their sentinel."""
    A = 4  # floats: 16 bytes
    base, _, _ = _los_call(name, "fwd", 500, (A, A, A))
    want, g_want = L.los_reference(name, 500, 512.0)
    assert abs(float(base) - want) <= LOS_TOL * want
    for offs in ((1, 1, A), (1, A, A), (A, 1, A)):
        loss, _, _ = _los_call(name, "fwd", 500, offs)
        print(f"{name} forward, offsets {offs}: loss {float(loss):.9g}, aligned {float(base):.9g}")
        assert abs(float(loss) - want) <= LOS_TOL * want
        assert torch.equal(loss.view(torch.int32), base.view(torch.int32)), offs
    _, buf0, at0 = _los_call(name, "bwd", 500, (A, A, A))
    assert float(np.abs(buf0[at0].cpu().numpy() - g_want.reshape(-1)).max()) <= LOS_TOL * float(np.abs(g_want).max())
    for offs in ((A, A, A), (1, 1, 1), (1, A, A), (A, 1, A), (A, A, 1)):
        _, buf, at = _los_call(name, "bwd", 500, offs)
        assert torch.equal(buf[at].view(torch.int32), buf0[at0].view(torch.int32)), offs
        guards = torch.cat([buf[:at.start], buf[at.stop:]])
        assert guards.numel() == 8 and bool((guards == 7.5).all()), offs


@pytest.mark.parametrize("name", ["40x768", "8197x8"])
def test_same_input_same_bits(name):
    w, z, d = _dev(name)
    a, ga = _run(w, z, d, 500, 512.0)
    torch.empty(1 << 20, device=DEV).fill_(float("nan"))  # (the workspace of the second call is not the first call's, nor clean)
    b, gb = _run(w, z, d, 500, 512.0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))


# ---- primary losses -----------------------------------------------------------------------------------------------------------------
OUTPUTS = ("loss", "g_depth", "g_image", "pts", "gt32")


def _fused(host, kinds, alphas, smooth, S):
    from lidar4d_amd import ops
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    out = ops.primary_losses_any(*dev, kinds, *alphas, smooth, L.DELTA, S, want_points=True, want_gt32=True)
    return {k: v.cpu().numpy() for k, v in zip(OUTPUTS, out)}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F32 and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("n", L.PRIMARY_N)
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_primary_losses_without_bce_have_the_emulations_bits(half, n):
    """The 27 triples of l1 / mse / huber on fp32 and fp16 ground truth, with the planted rows (dropped rays, e == 0, |e| == delta
    on both signs and a lattice step to either side, saturating predictions) and smooth in {0, 0.1, 0.2, 0.5}: loss, both
    gradients, both point sets and the fp32 copy of the ground truth bit for bit."""
    for smooth, alphas in L.SETTINGS:
        host = L.primary_inputs(n, half, n, smooth)
        *arrays, S = host
        for kinds in L.BCE_FREE:
            want = L.primary_losses_emul(*arrays, kinds, alphas, smooth, L.DELTA, S)
            got = _fused(arrays, kinds, alphas, smooth, S)
            for name in OUTPUTS:
                assert _same_bits(got[name], want[name]), (kinds, smooth, name, got[name], want[name])


@pytest.mark.parametrize("n", L.PRIMARY_N)
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_primary_losses_with_bce_vs_float64(half, n):
    """The 37 triples with BCE somewhere: bit-equal wherever no transcendental is involved, within four times the emulation's
    own measured deviation from float64 elsewhere (module docstring), and finite everywhere."""
    unit = 2.0 ** -24
    worst = dict.fromkeys(L.BCE_DEVIATION, 0.0)
    for smooth, alphas in L.SETTINGS:
        *arrays, S = L.primary_inputs(n, half, n, smooth)
        for kinds in L.WITH_BCE:
            args = (*arrays, kinds, alphas, smooth, L.DELTA, S)
            emul, ref, got = L.primary_losses_emul(*args), L.primary_losses_ref64(*args), _fused(arrays, kinds, alphas, smooth, S)
            assert all(np.isfinite(got[k]).all() for k in OUTPUTS), (kinds, smooth)
            assert _same_bits(got["pts"], emul["pts"]) and _same_bits(got["gt32"], emul["gt32"]), (kinds, smooth)
            feeds = {"loss": [True], "g_depth": [kinds[0] == "bce"], "g_image": [kinds[1] == "bce", kinds[2] == "bce"]}
            for name, cols in feeds.items():
                top = float(np.abs(ref[name]).max())
                g, e, r = (a[name].reshape(len(arrays[0]) if name != "loss" else 1, -1) for a in (got, emul, ref))
                for c, transcendental in enumerate(cols):
                    if not transcendental:
                        assert _same_bits(np.ascontiguousarray(g[:, c]), np.ascontiguousarray(e[:, c])), (kinds, smooth, name, c)
                        continue
                    err = float(np.abs(g[:, c].astype(F64) - r[:, c]).max())
                    worst[name] = max(worst[name], err / (unit * top) if err else 0.0)
                    assert err <= 4 * L.BCE_DEVIATION[name] * unit * top, (kinds, smooth, name, c, err / (unit * top))
    print(f"n = {n}, {'fp16' if half else 'fp32'}: largest deviation from float64 in units of 2^-24 of the output's largest magnitude: "
          + ", ".join(f"{k} {v:.2f} (bound {4 * L.BCE_DEVIATION[k]:.1f})" for k, v in worst.items()))


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_saturated_logits_give_exact_values(half):
    """BCE on all three terms at the planted logits: where the fp32 sigmoid in front of the ray-drop term is exactly 0 or 1 (from
    |logit| = 104, where expf(-|a|) is 0 and expf(-a) inf) the chain factor (1 - p) p is exactly 0 and so is the ray-drop
    gradient; the depth term's d / d a = sigmoid(a) - b is exactly 1 - b and 0 - b at a = +-1000."""
    smooth, alphas = L.SETTINGS[0]
    *arrays, S = L.primary_inputs(257, half, 1, smooth)
    depth, image, gt = arrays[:3]
    got = _fused(arrays, ("bce", "bce", "bce"), alphas, smooth, S)
    assert all(np.isfinite(got[k]).all() for k in OUTPUTS)
    rows = np.arange(L.LOGIT_ROWS.start, L.LOGIT_ROWS.stop)
    sat = rows[np.abs(image[rows, 0]) >= 104.0]
    assert sat.size == 8 and (got["g_image"][sat, 0] == 0).all()
    assert (got["g_image"][rows[(image[rows, 0] >= -20.0) & (image[rows, 0] < 16.0)], 0] != 0).all()
    hit = rows[: len(L.LOGITS)]  # m == 1, gt depth 0.5
    a_d = F32(alphas[0])
    assert float(got["g_depth"][hit[depth[hit] == 1000.0]][0]) == float(a_d * (F32(1.0) - F32(0.5)))
    assert float(got["g_depth"][hit[depth[hit] == -1000.0]][0]) == float(a_d * (F32(0.0) - F32(0.5)))
    assert (got["g_depth"][rows[len(L.LOGITS):]] == 0).all()  # m == 0


# ---- ray batch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
def test_ray_batch_outside_the_frame(tmp_path, fp16):
    """Rows above and below the frame (top = -1, -3, H - 1, H with patches 2 and 3 rows tall) and columns whose C remainder is
    negative or that wrap more than once (left = -1, -W - 2, W - 1, 2 W + 3 with 8 columns): include/lidar4d_step.h promises
    inds = row * W + column with the column mod W, and for a row outside [0, H) no pixel read and a ground truth of 0.  The torch
    route cannot index there; the reference is ray_batch_ref64."""
    import realdata_cases as rc
    from lidar4d_amd import ops
    ds = rc.fixture_dataset(tmp_path, "train", device=DEV, fp16=fp16)
    H, W = ds.H_lidar, ds.W_lidar
    top, left = [-1, -3, H - 1, H], [-1, -W - 2, W - 1, 2 * W + 3]
    fov = [float(v) for v in ds.intrinsics_lidar]
    for k, px in ((0, 2), (1, 3)):
        image, pose = ds.images_lidar[k], ds.poses_lidar[k]
        assert image.dtype == (torch.float16 if fp16 else torch.float32)
        out = ops.ray_batch_patches(torch.tensor(top, device=DEV), torch.tensor(left, device=DEV), (px, 8), pose, fov, H, W, image)
        rays_o, rays_d, gt, inds = (t[0].cpu().numpy() for t in out)
        host = (pose.cpu().numpy(), fov, H, W, image.cpu().numpy())
        w_inds, w_o, w_d, w_gt = L.ray_batch_ref64(top, left, px, 8, *host)
        rows = w_inds // W
        outside = (rows < 0) | (rows >= H)
        assert outside.any() and not outside.all() and w_inds.min() < 0 and w_inds.max() >= H * W
        assert np.array_equal(inds, w_inds) and gt.dtype == w_gt.dtype and np.array_equal(gt, w_gt) and not gt[outside].any()
        assert gt[~outside].any() and np.array_equal(rays_o, w_o)
        err = float(np.abs(rays_d - w_d).max())
        pi32 = float(np.abs(rays_d - L.ray_batch_ref64(top, left, px, 8, *host, pi=L.PI32)[2]).max())
        print(f"px = {px}: directions within {err:.2e} of the float64 reference ({pi32:.2e} with the float32 pi)")
        assert err <= 2e-7
