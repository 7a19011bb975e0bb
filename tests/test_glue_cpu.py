"""CPU tests of the references in tests/glue_cases.py, which tests/test_gpu_glue_ops.py compares the HIP kernels with: that every
lattice is exact (the references assert it while they are evaluated here), that the X-class inputs keep their near-boundary cases
below the cap, that the planes inputs leave enough samples for d/dxt, and that the references say what the model's torch
formulation says (the attribute glue of lidar4d.py, trunc_exp of activation.py, the scene-flow loss of runner.py:222-253)."""
import numpy as np
import pytest
import torch

import glue_cases as gc

F16, F32, F64 = np.float16, np.float32, np.float64


# ---- X class --------------------------------------------------------------------------------------------------------------------
def test_x_classify_marks_midpoints_and_nothing_else():
    h = np.array([1.0, 1.0 + 2.0 ** -10, 0.0, 65504.0, 6.0e-8], F16).astype(F64)
    mid = np.array([1.0 + 2.0 ** -11, 2.0 ** -25, 65520.0, 1.5 * 2.0 ** -24])
    for v in (mid, mid * (1 + 7 * 2.0 ** -24), mid * (1 - 7 * 2.0 ** -24), -mid):
        want, other, near, dist = gc.x_classify(v)
        assert near.all() and (dist <= 7.01).all()
        assert (np.abs(want.astype(F64) - other.astype(F64))[:2] > 0).all() and not gc.same_bits(want, other).any()
    want, other, near, _ = gc.x_classify(np.array([65520.0 * (1 - 2.0 ** -22)]))
    assert want[0] == F16(65504.0) and np.isinf(other[0]) and near[0]
    for v in (h, mid * (1 + 9 * 2.0 ** -24), mid * (1 - 9 * 2.0 ** -24), np.array([0.3, -7.7, 1e-3, 70000.0, 1e-12])):
        assert not gc.x_classify(v)[2].any()
    with pytest.raises(AssertionError):  # one fp16 ulp off, away from any midpoint
        gc.x_check(np.array([1.0 + 2.0 ** -10], F16), np.array([1.0 + 2.0 ** -13]), "probe")
    with pytest.raises(AssertionError):  # near a midpoint, but two values away
        gc.x_check(np.array([1.0 + 2.0 ** -9], F16), np.array([1.0 + 2.0 ** -11]), "probe")
    assert gc.x_check(np.array([1.0 + 2.0 ** -10] + [0.5] * 999, F16), np.array([1.0 + 2.0 ** -11] + [0.5] * 999), "probe")[0] == 1


def test_x_class_near_boundary_cases_stay_below_the_cap():
    x = gc.all_f16()
    fin = np.isfinite(x)
    assert int(fin.sum()) == 63488
    near = gc.x_classify(gc.sigmoid64(x[fin]))[2]
    print(f"sigmoid: {int(near.sum())} near-boundary cases of {near.size}")
    assert near.sum() <= gc.X_CAP * 65536 and near.sum() == 60
    d = gc.sigma_d_pow2(65536)
    assert (np.abs(d) == np.exp2(np.round(np.log2(np.abs(d))))).all() and (d > 0).any() and (d < 0).any()
    assert set(np.round(np.log2(np.abs(d))).astype(int)) == set(range(-14, 4))
    v = gc.trunc_exp_bwd64(x[fin], d[fin], 128.0)
    near = gc.x_classify(v)[2]
    print(f"exp * 2^k, k per row: {int(near.sum())} near-boundary cases of {near.size}")
    assert near.sum() <= gc.X_CAP * 65536
    with np.errstate(over="ignore"):
        assert np.isinf(v.astype(F16)).any() and (v.astype(F16) == 0).any()  # the rows reach both ends of fp16
    for k in range(-14, 4):  # and for any single k
        near = gc.x_classify(gc.trunc_exp_bwd64(x[fin], 2.0 ** k, 128.0))[2]
        assert near.sum() <= gc.X_CAP * 65536, k


def test_small_sigma_cases_have_no_near_boundary_case():
    for P in gc.SIGMA_SMALL_P:
        h0, d = gc.sigma_small_case(P)
        assert h0.shape == d.shape == (P,) and not gc.x_classify(gc.trunc_exp_bwd64(h0, d, 128.0))[2].any()
        assert P == 1 or ((np.abs(h0) > 15).any() and (np.abs(h0) < 15).any())


def test_trunc_exp_reference_is_the_oracles():
    from oracle.fields_ref import _TruncExp
    x = gc.all_f16()
    x = x[~np.isnan(x)]
    d = gc.sigma_d_pow2(x.size)
    leaf = torch.from_numpy(x.astype(F64)).requires_grad_(True)
    # (_TruncExp works in fp32: its forward is compared through fp32, its adjoint at fp32 accuracy)
    out = _TruncExp.apply(leaf)
    out.backward(torch.from_numpy(d))
    with np.errstate(over="ignore"):
        want = np.exp(x.astype(F64))
        assert np.allclose(out.detach().numpy().astype(F64)[np.isfinite(x)], want.astype(F32).astype(F64)[np.isfinite(x)], rtol=4e-7, atol=0, equal_nan=True)
    ref = gc.trunc_exp_bwd64(x, d, 1.0)
    assert np.allclose(leaf.grad.numpy(), ref, rtol=4e-7, atol=0)
    assert ref[x == F16(np.inf)][0] == d[x == F16(np.inf)][0] * np.exp(15.0) and np.isfinite(ref).all()


# ---- attribute glue -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_enc,n_geo,in_pad", [(64, 15, 96), (66, 15, 96), (16, 3, 32), (0, 15, 16), (8, 0, 16)])
def test_gather_reference_is_index_and_concat(n_enc, n_geo, in_pad):
    c = gc.gather_case(n_enc, n_geo, in_pad, cap=37, T=7, with_idx=True)
    idx = torch.from_numpy(c["idx"]).long()
    d = torch.from_numpy(c["dir_enc"])[idx // c["T"]]
    geo = torch.from_numpy(c["h"])[idx, 1:1 + n_geo]
    want = torch.cat([d, geo, torch.ones(37, in_pad - n_enc - n_geo, dtype=torch.float16)], -1).numpy()
    assert gc.same_bits(gc.attr_gather_ref(c, None), want).all() and not np.isnan(want).any()
    part = gc.attr_gather_ref(c, 20)
    assert gc.same_bits(part[:20], want[:20]).all() and (part[20:] == gc.SENTINEL16).all()
    assert gc.same_bits(gc.attr_gather_ref(c, 99), want).all() and (gc.attr_gather_ref(c, 0) == gc.SENTINEL16).all()


def test_scatter_and_gather_adjoints_are_the_float64_autograd():
    """sigmoid -> .half() -> scatter, and index -> concat, as torch float64 graphs: their gradients against the E references at
    inputs where fp32 / fp16 round nothing away (so the comparison needs only the final rounding's tolerance)."""
    r = gc.rng_of(31)
    cap, P = 50, 80
    idx = gc.work_list(P, cap, (1,))
    y = torch.from_numpy(r.uniform(-2, 2, size=(cap, 2))).requires_grad_(True)
    s = torch.sigmoid(y)
    dense = torch.zeros(P, 2, dtype=torch.float64)
    dense[torch.from_numpy(idx).long()] = s
    d_attr = r.uniform(-1, 1, size=(P, 2)).astype(F32)
    (dense * torch.from_numpy(d_attr.astype(F64))).sum().backward()
    s16 = s.detach().numpy().astype(F16)  # what the forward stores: sigmoid(...).half()
    assert gc.same_bits(s16, gc.sigmoid64(y.detach().numpy()).astype(F16)).all()
    got_r, got_i = gc.attr_scatter_bwd_ref(d_attr, s16.astype(F32), idx, 128.0)
    for c, got in enumerate((got_r, got_i)):
        want = y.grad.numpy()[:, c] * 128.0
        assert np.allclose(got[:, 0].astype(F64), want, rtol=3e-3, atol=1e-3) and (got[:, 1:] == 0).all() and not np.signbit(got[:, 1:]).any()
    # gather: d/dh[idx[j], 1 + k] = dxa_r[j, n_enc + k] + dxa_i[j, n_enc + k]
    in_pad, n_enc, n_geo = 32, 16, 15
    c = gc.gather_bwd_case(in_pad, n_enc, n_geo, cap, P)
    for k in ("dxa_r", "dxa_i"):
        c[k][0, n_enc:n_enc + 4] = F16(1.0)  # (the planted overflows are the GPU test's business)
    h = torch.zeros(P, 16, dtype=torch.float64, requires_grad=True)
    rows = torch.cat([torch.zeros(cap, n_enc, dtype=torch.float64), h[torch.from_numpy(c["idx"]).long(), 1:1 + n_geo],
                      torch.ones(cap, 1, dtype=torch.float64)], -1)
    ((rows * torch.from_numpy(c["dxa_r"].astype(F64))).sum() + (rows * torch.from_numpy(c["dxa_i"].astype(F64))).sum()).backward()
    got = gc.attr_gather_bwd_ref(c, in_pad, n_enc, n_geo, 0, rows_kernel=True)
    touched = np.zeros(P, bool)
    touched[c["idx"]] = True
    assert np.allclose(got[touched].astype(F64), h.grad.numpy()[touched], rtol=2.0 ** -10, atol=0)
    assert (got[~touched] == gc.SENTINEL16).all() and (got[touched, 0] == 0).all()
    shifted = gc.attr_gather_bwd_ref(c, in_pad, n_enc, n_geo, 1, rows_kernel=True)  # h_layout: the same columns one further right
    c2 = dict(c, dxa_r=np.roll(c["dxa_r"], -1, axis=1), dxa_i=np.roll(c["dxa_i"], -1, axis=1))
    assert gc.same_bits(shifted, gc.attr_gather_bwd_ref(c2, in_pad, n_enc, n_geo, 0, rows_kernel=True)).all()
    generic = gc.attr_gather_bwd_ref(c, in_pad, n_enc, 7, 0, rows_kernel=False)
    assert (generic[:, 0] == gc.SENTINEL16).all() and (generic[:, 8:] == gc.SENTINEL16).all()


# ---- scene-flow glue ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", gc.FLOW_GRAD_SHAPES + [(300, 299)])
def test_flow_chamfer_lattice_is_exact(n, m):
    c = gc.flow_grad_case(n, m, same_neighbour=(n, m) == (300, 299))
    dy = c["dy0"].astype(F64)
    for t in c["terms"]:
        part = gc.flow_chamfer_grad_ref(t, dy)  # asserts the lattice
        assert part.shape == ((max(n, m) + 255) // 256,)
        gc.to_f32_exact(part)
        assert part.sum() == t["dist1"].astype(F64).sum() + t["dist2"].astype(F64).sum()
    gc.to_f32_exact(dy)
    assert (dy[:, :3] != c["dy0"][:, :3]).any() and (dy[:, 3:] != c["dy0"][:, 3:]).any()
    if (n, m) == (300, 299):
        assert all((t["idx2"] == 0).all() for t in c["terms"])


def test_flow_loss_finish_lattice_is_exact():
    for n_partial in gc.FINISH_PARTIALS:
        for ng in gc.FINISH_GROUND:
            c = gc.finish_case(n_partial, ng, 6 * 37 + (ng & 1))
            loss, dy_g, amax, bound = gc.flow_loss_finish_ref(c, gc.W_GROUND_LATTICE)  # asserts the lattice
            assert bound == 0.0 and float(F32(loss)) == loss and amax[0] == F32(7.25)
            if ng:
                y = c["y_g"][:, :6]
                assert np.isnan(c["y_g"][:, 6:]).all() and (y > 0).any() and (y < 0).any()
                assert (np.signbit(y) & (y == 0)).any() and (~np.signbit(y) & (y == 0)).any()
                assert (dy_g[y == 0] == 0).all() and not np.signbit(dy_g[y == 0]).any()
                assert set(np.unique(dy_g)) == {F32(-2.0 ** -10), F32(0.0), F32(2.0 ** -10)}
            else:
                assert dy_g is None and amax[1] == 0 and loss == (3.5 if n_partial else 0.0)


def test_dy16_scales_cover_the_issue():
    kinds = [k for _, _, k in gc.dy16_scales()]
    assert kinds.count("clamp+") == 3 and kinds.count("clamp-") == 1 and kinds.count("edge") >= 21 and kinds.count("k") >= 4
    assert any(g < 0 for _, g, _ in gc.dy16_scales())
    out = gc.dy16_ref(np.array([[1.0, -2.0, 0.5, 3.0, 1e5, 0.0]], F32), F32(-3.0), 4)
    assert out.shape == (1, 16) and out[0, 0] == F16(-48.0) and np.isinf(out[0, 4]) and out[0, 4] < 0 and not out[0, 6:].any()


def test_axpy_reference_keeps_bits_where_x_is_zero():
    y, x, a = gc.axpy_case(257)
    out = gc.axpy_ref(y, x, a)
    assert np.isnan(out[3]) and np.isnan(out[256]) and np.signbit(out[4]) and out[4] == 0 and np.signbit(out[5])
    assert gc.same_bits(out[x == 0], y[x == 0]).all() and (out[x != 0] != y[x != 0]).all() and (x == 0).sum() > 50


def test_float64_pieces_reproduce_the_runner_formula():
    """trainer.flow_loss / runner.py:222-253 as a torch float64 autograd graph (cdist-free brute force, argmin detached as the
    chamfer op's backward does) against the composition of the pieces the kernels compute: value and d / d(flow output)."""
    n, m, ng = 300, 700, 50
    r = gc.rng_of(41)
    pc = r.uniform(-1, 1, size=(n, 3))
    y, y_g = r.uniform(-0.05, 0.05, size=(n, 6)), r.uniform(-0.05, 0.05, size=(ng, 6))
    others = [(r.uniform(-1, 1, size=(m - 13 * v, 3)), float(step), col0) for v, (step, col0) in enumerate(((1, 0), (1, 3), (2, 0), (2, 3)))]
    yt, ygt, pct = torch.from_numpy(y).requires_grad_(True), torch.from_numpy(y_g).requires_grad_(True), torch.from_numpy(pc)
    pred = {"forward": yt[:, :3], "backward": yt[:, 3:]}
    loss = pct.new_zeros(())
    for q, step, col0 in others:
        pc_pred = pct + pred["forward" if col0 == 0 else "backward"] * step
        d = ((pc_pred[:, None, :] - torch.from_numpy(q)[None, :, :]) ** 2).sum(-1)
        loss = loss + (d.min(1).values.sum() + d.min(0).values.sum()) * 0.5
    loss = loss + 0.001 * (ygt[:, :3].abs().sum() + ygt[:, 3:].abs().sum())
    loss.backward()
    got, dy, dy_g = gc.flow_loss_pieces64(pc, y, others, y_g)
    assert abs(got - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert np.abs(dy - yt.grad.numpy()).max() <= 1e-12 * np.abs(dy).max() and np.abs(dy).max() > 0.1
    assert np.array_equal(dy_g, ygt.grad.numpy())


# ---- chamfer --------------------------------------------------------------------------------------------------------------------
def test_nn_reference_rule():
    """strict <, first minimum, 3.4e38 start: ties, NaN / inf queries and candidates, against a scalar loop."""
    a = np.array([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [1, 1, 1], [3e19, 0, 0]], F32)
    b = np.array([[1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1]], F32)
    dist, idx = gc.nn_ref(a, b)
    want_d, want_i = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for p in a:
            best, bi = gc.CHAMFER_START, 0
            for j, q in enumerate(b):
                dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                d = (dx * dx + dy * dy) + dz * dz
                if d < best:
                    best, bi = d, j
            want_d.append(best), want_i.append(bi)
    assert gc.same_bits(dist, np.array(want_d, F32)).all() and (idx == np.array(want_i)).all()
    assert list(idx) == [3, 0, 0, 5, 0] and dist[1] == gc.CHAMFER_START and dist[2] == gc.CHAMFER_START and dist[4] == gc.CHAMFER_START


@pytest.mark.parametrize("b,n,m", gc.CHAMFER_SHAPES)
def test_chamfer_cases_hold_their_plants(b, n, m):
    xyz1, xyz2 = gc.chamfer_case(b, n, m)
    d1, d2, i1, i2 = gc.chamfer_ref(xyz1, xyz2)
    segs, seg_len = gc.seg_for(n, m, b)
    assert ((b, n, m) in gc.CHAMFER_MULTI_SEGMENT) == (segs > 1)
    J = gc.plant_indices(m)
    if J:
        assert (d1[:, 0] == 0).all() and (i1[:, 0] == J[0]).all()  # a query equal to a candidate: the smallest index of the copies
        tile = lambda j: (j // seg_len, (j % seg_len) // 1024)
        if segs > 2:
            assert tile(J[0]) == tile(J[1]) and J[0] // seg_len != J[2] // seg_len
        elif segs == 2:
            assert J[0] // seg_len != J[2] // seg_len or J[0] // seg_len != J[1] // seg_len
    if (b, n, m) == (1, 300, 3000):
        assert (segs, seg_len) == (3, 1000) and J == [1500, 1510, 2500]
        # natural ties on the lattice: queries whose minimum is attained by several candidates
        d = ((xyz2[0][None] - xyz1[0][:, None]).astype(F64) ** 2).sum(-1)
        assert ((d == d.min(1, keepdims=True)).sum(1) > 1).sum() >= 20
    if n >= 12:
        assert (d2[:, 0] == 0).all() and (i2[:, 0] == gc.plant_indices(n)[0]).all()


def test_chamfer_backward_lattice_is_exact():
    for (n, m) in ((300, 3), (3, 300), (257, 255)):
        xyz1, xyz2 = gc.lattice_cloud(n, 4, (n, m, 1))[None], gc.lattice_cloud(m, 4, (n, m, 2))[None]
        _, _, i1, i2 = gc.chamfer_ref(xyz1, xyz2)
        gd1 = (gc.rng_of(43, n).randint(-8, 9, size=(1, n)) / 4.0).astype(F32)
        gd2 = (gc.rng_of(47, m).randint(-8, 9, size=(1, m)) / 4.0).astype(F32)
        g1, g2 = gc.chamfer_bwd_ref(xyz1, xyz2, gd1, gd2, i1, i2, np.full((1, n, 3), 0.25, F32), np.full((1, m, 3), -0.5, F32))
        gc.to_f32_exact(g1), gc.to_f32_exact(g2)
        if min(n, m) == 3:  # many queries share one neighbour
            assert np.bincount((i1 if n > m else i2)[0], minlength=3).max() >= 100


# ---- planes ---------------------------------------------------------------------------------------------------------------------
def test_planes_inputs_leave_enough_samples_for_dxt():
    assert gc.planes_resolutions() == [[6, 10, 12, 5], [18, 30, 36, 5]]
    xt = gc.planes_xt()
    assert xt.shape[0] > 2049 and xt.dtype == F32 and xt.min() < 0 and xt.max() > 1
    ok = gc.planes_dxt_mask(xt)
    print(f"planes: {int(ok.sum())} of {ok.size} samples qualify for d/dxt")
    assert ok.mean() >= 0.95 and not ok[2049:].all()
    assert ((xt == 0).any(1) & (xt == 1).any(1)).any()
    assert gc.planes_xt(1).shape == (1, 4)
