"""Edge-shape tests of ray sampling and compositing on the device (``-m gpu``, MI355X): sample_rays_kernel and the dense
sample_rays_xt_kernel, composite_fwd_kernel with its mask and work list, composite_image_kernel and composite_bwd_kernel, each
against a reference that no HIP code computed (tests/render_cases.py).

Every test names its kind of reference: E (sampling re-evaluated in numpy fp32, bit-equal), S (saturated lattice: alpha exactly 0
or 1, closed forms, equal values) or N (float64 reference, the project's tolerances, each shown on the CPU to hold for a float32
restatement with a factor four to spare).  The rules, the cases and why they are these: tests/render_cases.py; the references
themselves: tests/test_render_cpu.py."""
import numpy as np
import pytest
import torch

import render_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64
SENT = F32(-12345.0)
WORST = {}  # largest excess over the rtol term seen so far, per output (printed: tests/render_cases.py records them)


def _ops():
    from lidar4d_amd import ops
    return ops


def _err():
    from lidar4d_amd._lib import HipExtensionError
    return HipExtensionError


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def assert_bits(got, want, what):
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    same = rc.same_bits(got, want) if got.dtype.kind == "f" else got == want
    bad = np.flatnonzero(~same.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[:6]}: got {got.reshape(-1)[bad[:6]]}, want {want.reshape(-1)[bad[:6]]}"


def fwd(c, want_mask=True, want_idx=True):
    """ops.composite_fwd of a case.  -> dict of numpy arrays (absent outputs None), '_w' the device weights."""
    w, ws, d, m, idx, cnt = _ops().composite_fwd(dev(c["sigma"]), dev(c["z"]), c["sample_dist"], c["density_scale"], c["active"],
                                                 want_mask=want_mask, want_idx=want_idx)
    return dict(weights=host(w), weights_sum=host(ws), depth=host(d), mask=host(m), idx=host(idx),
                count=None if cnt is None else int(cnt), _w=w)


def bwd(c, w_dev, attr, C, grads, want_d_attr=True):
    """ops.composite_bwd.  grads: dict, None = null pointer.  -> d_sigma, d_attr as numpy."""
    ds, da = _ops().composite_bwd(dev(c["sigma"]), dev(c["z"]), w_dev, dev(attr), C, c["sample_dist"], c["density_scale"], c["active"],
                                  dev(grads.get("d_depth")), dev(grads.get("d_wsum")), dev(grads.get("d_image")),
                                  dev(grads.get("d_weights")), want_d_attr=want_d_attr)
    assert (da is None) == (not want_d_attr)
    return host(ds), host(da)


def note(key, value):
    WORST[key] = max(WORST.get(key, -np.inf), value)
    return WORST[key]


# =================================================================================================================================
# 1. sampling
# =================================================================================================================================
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("N,T", rc.SAMPLE_SHAPES)
def test_sampling_bits(N, T, with_noise):
    """E.  z_vals of l4d_sample_rays (with and without xyz) and of the dense l4d_sample_rays_xt, xyz, and the four columns of xt:
    the t column carries t's bits, a clamped coordinate is exactly 0 or 1.  lin as the renderer builds it."""
    ops = _ops()
    lin = torch.linspace(0.0, 1.0, T, device=DEV)
    assert lin.shape == (T,) and float(lin[0]) == 0.0
    t_dev = dev(np.array([rc.SAMPLE_T], F32))
    for c in rc.sample_cases(N, T, with_noise):
        z_ref, xyz_ref, xt_ref, beyond = rc.sample_ref(c["rays_o"], c["rays_d"], host(lin), c["noise"], c["near"], c["far"], c["bound"])
        what = f"N={N} T={T} bound={c['bound']} noise={with_noise}"
        ro, rd, noise = dev(c["rays_o"]), dev(c["rays_d"]), dev(c["noise"])
        z, xyz = ops.sample_rays(ro, rd, lin, noise, c["near"], c["far"], c["bound"])
        assert_bits(z, z_ref, "sample_rays z_vals " + what)
        assert_bits(xyz, xyz_ref, "sample_rays xyz " + what)
        z, none = ops.sample_rays(ro, rd, lin, noise, c["near"], c["far"], c["bound"], want_xyz=False)
        assert none is None
        assert_bits(z, z_ref, "sample_rays z_vals alone " + what)
        z, xt = ops.sample_rays_xt(ro, rd, lin, noise, t_dev, c["near"], c["far"], c["bound"])
        assert_bits(z, z_ref, "sample_rays_xt z_vals " + what)
        assert_bits(xt, xt_ref, "sample_rays_xt xt " + what)
        xt, b = host(xt), beyond.reshape(-1, 3)
        assert_bits(xt[:, 3], np.full(N * T, rc.SAMPLE_T, F32), "xt: column 3 carries t")
        assert (b != 0).any() and (xt[:, :3][b == 1] == 1.0).all() and (xt[:, :3][b == -1] == 0.0).all()


# =================================================================================================================================
# 2. compositing structure
# =================================================================================================================================
@pytest.mark.parametrize("active", [False, True])
@pytest.mark.parametrize("N,T", rc.STRUCT_SHAPES)
def test_structure_one_opaque_sample(N, T, active):
    """S.  Forward (one-hot weights, mask and work list, weights_sum 1, depth z_p), image (attr[r, p_r]) and adjoint with C = 2 and
    every gradient present ((g_i - g_p) c, 0, fl32(g_i 1e-15f) c; d_attr = weights (x) d_image)."""
    c = rc.struct_inputs(N, T, active)
    attr, grads = rc.struct_attr(N, T, 2), rc.struct_grads(N, T, 2)
    f = fwd(c)
    rc.struct_check_fwd(c, f)
    image = _ops().composite_image(f["_w"], dev(attr), 2)
    rc.assert_values(host(image), rc.struct_image_ref(c, attr, 2), f"image N={N} T={T}")
    d_sigma, d_attr = bwd(c, f["_w"], attr, 2, grads)
    rc.struct_check_bwd(c, attr, 2, grads, d_sigma, d_attr)


@pytest.mark.parametrize("active", [False, True])
@pytest.mark.parametrize("T", sorted(rc.STRUCT_MULTI))
def test_structure_two_and_three_opaque_samples(T, active):
    """S.  Opaque samples in different chunks and segments: weights 1, 1e-15f, fl32(1e-15f 1e-15f) -- the transmittance carried
    from chunk to chunk and from segment to segment; only the first is in the mask and the list."""
    c = rc.struct_inputs(len(rc.STRUCT_MULTI[T]), T, active, rc.STRUCT_MULTI[T])
    rc.struct_check_fwd(c, fwd(c))


@pytest.mark.parametrize("T", [65, 1025])
def test_structure_widths_and_null_gradients(T):
    """S.  C = 0 with attr = None (the renderer's call), 1, 3, 4; each upstream gradient null in turn; all four null; no d_attr."""
    N = 17
    c = rc.struct_inputs(N, T, True)
    f = fwd(c)
    for C in (0, 1, 3, 4):
        attr = rc.struct_attr(N, T, C) if C else None
        grads = rc.struct_grads(N, T, C)
        if not C:
            grads["d_image"] = None
        d_sigma, d_attr = bwd(c, f["_w"], attr, C, grads, want_d_attr=bool(C))
        rc.struct_check_bwd(c, attr, C, grads, d_sigma, d_attr, want_d_attr=bool(C))
    attr, full = rc.struct_attr(N, T, 2), rc.struct_grads(N, T, 2)
    for drop in ("d_depth", "d_wsum", "d_image", "d_weights"):
        grads = dict(full, **{drop: None})
        d_sigma, d_attr = bwd(c, f["_w"], attr, 2, grads)
        rc.struct_check_bwd(c, attr, 2, grads, d_sigma, d_attr)
    none = dict.fromkeys(full)
    d_sigma, d_attr = bwd(c, f["_w"], attr, 2, none)
    rc.struct_check_bwd(c, attr, 2, none, d_sigma, d_attr)
    assert (d_sigma == 0).all() and (d_attr == 0).all()
    d_sigma, d_attr = bwd(c, f["_w"], attr, 2, full, want_d_attr=False)
    rc.struct_check_bwd(c, attr, 2, full, d_sigma, None, want_d_attr=False)


@pytest.mark.parametrize("T", [65, 1025])
def test_output_flags_do_not_change_the_outputs(T):
    """The four combinations of want_mask and want_idx: the same bits of weights, weights_sum and depth (S and N inputs)."""
    for c in (rc.struct_inputs(17, T, False), rc.numeric_case(rc.NUMERIC_N, T, True, 2)):
        base = fwd(c)
        for want_mask in (False, True):
            for want_idx in (False, True):
                f = fwd(c, want_mask, want_idx)
                assert (f["mask"] is None) == (not want_mask) and (f["idx"] is None) == (not want_idx)
                for k in ("weights", "weights_sum", "depth"):
                    assert_bits(f[k], base[k], f"{k} want_mask={want_mask} want_idx={want_idx}")
                if want_mask:
                    assert_bits(f["mask"], base["mask"], "mask")
                if want_idx:
                    assert f["count"] == base["count"]
                    assert_bits(np.sort(f["idx"][:f["count"]]), np.sort(base["idx"][:base["count"]]), "work list")


@pytest.mark.parametrize("T", rc.GUARD_T)
@pytest.mark.parametrize("N", rc.GUARD_N)
def test_guards_keep_the_row_behind_the_last_ray(N, T):
    """S, through the C ABI with buffers of N + 1 ray rows prefilled with a sentinel: the rays are as in the structural test, the
    spare row and the work list behind ``count`` keep the sentinel (a workgroup's wavefronts behind the last ray store nothing)."""
    ops = _ops()
    p = ops._p
    c = rc.struct_inputs(N, T, True)
    C, attr, grads = 2, rc.struct_attr(N, T, 2), rc.struct_grads(N, T, 2)
    sigma, z = dev(c["sigma"]), dev(c["z"])
    w, ws, d = filled((N + 1, T), SENT), filled((N + 1,), SENT), filled((N + 1,), SENT)
    mask = filled((N + 1, T), 7, torch.uint8)
    idx, cnt = filled(((N + 1) * T,), -7, torch.int32), filled((1,), -7, torch.int32)
    ops.call("l4d_composite_fwd", p(sigma), p(z), N, T, c["sample_dist"], c["density_scale"], 1, p(w), p(ws), p(d), p(mask), p(idx),
             p(cnt), ops._stream())
    got = dict(weights=host(w)[:N], weights_sum=host(ws)[:N], depth=host(d)[:N], mask=host(mask)[:N], idx=host(idx), count=int(cnt))
    rc.struct_check_fwd(c, got)
    assert_bits(w[N], np.full(T, SENT, F32), "weights: spare row")
    assert float(ws[N]) == SENT and float(d[N]) == SENT and bool((mask[N] == 7).all())
    assert got["count"] == N and bool((idx[N:] == -7).all()), "work list behind count"
    image = filled((N + 1, C), SENT)
    ops.call("l4d_composite_image", p(w), p(dev(attr)), N, T, C, p(image), ops._stream())
    rc.assert_values(host(image)[:N], rc.struct_image_ref(c, attr, C), "image")
    assert_bits(image[N], np.full(C, SENT, F32), "image: spare row")
    d_sigma, d_attr = filled((N + 1, T), SENT), filled(((N + 1) * T, C), SENT)
    g = {k: dev(v) for k, v in grads.items()}
    ops.call("l4d_composite_bwd", p(sigma), p(z), p(w), p(dev(attr)), N, T, C, c["sample_dist"], c["density_scale"], 1, p(g["d_depth"]),
             p(g["d_wsum"]), p(g["d_image"]), p(g["d_weights"]), p(d_sigma), p(d_attr), ops._stream())
    rc.struct_check_bwd(c, attr, C, grads, host(d_sigma)[:N], host(d_attr)[:N * T])
    assert_bits(d_sigma[N], np.full(T, SENT, F32), "d_sigma: spare row")
    assert_bits(d_attr[N * T:], np.full((T, C), SENT, F32), "d_attr: spare row")


def test_refusals_write_nothing():
    """C = 5 and T = 8193: the library's error from ops.composite_bwd, and a prefilled d_sigma untouched through the C ABI."""
    ops = _ops()
    p = ops._p
    for N, T, C in ((3, 65, rc.C_MAX + 1), (2, rc.T_MAX + 1, 2)):
        c = rc.struct_inputs(N, T, False)
        sigma, z = dev(c["sigma"]), dev(c["z"])
        w = filled((N, T), 0.0)
        attr, d_image, ones = filled((N * T, C), 0.5), filled((N, C), 1.0), filled((N,), 1.0)
        with pytest.raises(_err(), match="l4d_composite_bwd"):
            ops.composite_bwd(sigma, z, w, attr, C, c["sample_dist"], 1.0, False, ones, ones, d_image, w)
        d_sigma, d_attr = filled((N, T), SENT), filled((N * T, C), SENT)
        with pytest.raises(_err(), match="l4d_composite_bwd"):
            ops.call("l4d_composite_bwd", p(sigma), p(z), p(w), p(attr), N, T, C, c["sample_dist"], 1.0, 0, p(ones), p(ones), p(d_image),
                     p(w), p(d_sigma), p(d_attr), ops._stream())
        torch.cuda.synchronize()
        assert_bits(d_sigma, np.full((N, T), SENT, F32), "d_sigma of a refused call")
        assert_bits(d_attr, np.full((N * T, C), SENT, F32), "d_attr of a refused call")


# =================================================================================================================================
# 3. compositing numerics
# =================================================================================================================================
def check_work_list(f, N, T):
    """mask == (device weights > 1e-4), count == mask.sum(), idx[:count] without repeats and, as a set, nonzero(mask)."""
    mask = f["mask"].astype(bool)
    assert (mask == (f["weights"] > rc.MASK_THRESHOLD)).all(), "mask != (weights > 1e-4)"
    assert f["count"] == int(mask.sum())
    idx = f["idx"][:f["count"]]
    assert np.unique(idx).size == idx.size, "work list repeats a sample"
    assert np.array_equal(np.sort(idx), np.flatnonzero(mask.reshape(-1)).astype(np.int32)), "work list != nonzero(mask)"
    return idx


@pytest.mark.parametrize("N,T,active,C", rc.NUMERIC_CASES)
def test_numerics_against_float64(N, T, active, C):
    """N.  Forward, image and adjoint at well-conditioned inputs against the float64 reference; the mask may differ from the
    reference's only within the weights tolerance of the threshold."""
    c = rc.numeric_case(N, T, active, C)
    f64 = rc.composite_ref64(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], active, c["attr"], C)
    ds64, da64 = rc.composite_bwd_ref64(c, f64)
    f = fwd(c)
    f["image"] = host(_ops().composite_image(f["_w"], dev(c["attr"]), C))
    d_sigma, d_attr = bwd(c, f["_w"], c["attr"], C, c)
    ds_max = float(np.abs(ds64).max())
    seen = {k: rc.excess(f[k], f64[k], rc.TOL[k][0]) for k in ("weights", "weights_sum", "depth", "image")}
    seen["d_attr"] = rc.excess(d_attr, da64, rc.TOL["d_attr"][0])
    seen["d_sigma"] = rc.excess(d_sigma, ds64, rc.DSIGMA_RTOL) / ds_max
    idx = check_work_list(f, N, T)
    differ = f["mask"].astype(bool) != (f64["weights"] > float(rc.MASK_THRESHOLD))
    seen["mask_differs"] = int(differ.sum())
    print(f"N={N} T={T} active={active} C={C}: excess over the rtol term " + " ".join(f"{k}={v:+.2e}" for k, v in seen.items()) +
          " | largest so far " + " ".join(f"{k}={note(k, v):+.2e}" for k, v in seen.items()))
    for k in ("weights", "weights_sum", "depth", "image"):
        rc.assert_close(f[k], f64[k], *rc.TOL[k], what=k)
    rc.assert_close(d_attr, da64, *rc.TOL["d_attr"], what="d_attr")
    rc.assert_close(d_sigma, ds64, rc.DSIGMA_RTOL, rc.DSIGMA_K * ds_max, "d_sigma")
    assert not (differ & ~rc.borderline(f64["weights"])).any(), "the mask differs from the reference away from the threshold"
    assert idx.size > 0 or T == 1


@pytest.mark.parametrize("T", [t for t in rc.T_EDGES if t <= rc.SEGMENT])
def test_work_list_is_in_ray_order_within_one_workgroup_and_segment(T):
    """N <= 16 rays and T <= 1024: one atomicAdd reserves the slots, the wavefronts take their shares in ray order and write their
    chunks in order, so the list is strictly ascending."""
    for N in (5, rc.FWD_RAYS):
        f = fwd(rc.numeric_case(N, T, False, 2))
        idx = check_work_list(f, N, T)
        assert (np.diff(idx.astype(np.int64)) > 0).all(), "work list not ascending"
        assert idx.size > 0 or T == 1


# =================================================================================================================================
# 4. independence and non-finite input
# =================================================================================================================================
def _everything(c):
    f = fwd(c)
    f["image"] = host(_ops().composite_image(f["_w"], dev(c["attr"]), c["C"]))
    f["d_sigma"], f["d_attr"] = bwd(c, f["_w"], c["attr"], c["C"], c)
    return f


@pytest.mark.parametrize("active", [False, True])
def test_rays_do_not_depend_on_the_batch(active):
    """Rays 0, 15, 16 and 32 of a 33-ray batch at T = 1025 (first and last wavefront of the forward's first workgroup, first of its
    second, the single ray of its third; every slot of the adjoint's workgroups of 4) rendered alone: bit-equal.  And the same
    call twice gives the same bits."""
    N, T, C = 33, 1025, 2
    c = rc.numeric_case(N, T, active, C)
    a, b = _everything(c), _everything(c)
    for k in ("weights", "weights_sum", "depth", "mask", "image", "d_sigma", "d_attr"):
        assert_bits(a[k], b[k], k + " of the same call")
    assert a["count"] == b["count"]
    assert_bits(np.sort(a["idx"][:a["count"]]), np.sort(b["idx"][:b["count"]]), "work list of the same call")
    for r in (0, 15, 16, 32):
        one = _everything(rc.take_rays(c, [r]))
        for k in ("weights", "weights_sum", "depth", "mask", "image", "d_sigma"):
            assert_bits(one[k][0], a[k][r], f"{k} of ray {r} alone")
        assert_bits(one["d_attr"], a["d_attr"][r * T:(r + 1) * T], f"d_attr of ray {r} alone")
        in_ray = np.sort(a["idx"][:a["count"]])
        in_ray = in_ray[(in_ray >= r * T) & (in_ray < (r + 1) * T)] - r * T
        assert_bits(np.sort(one["idx"][:one["count"]]), in_ray.astype(np.int32), f"work list of ray {r} alone")


@pytest.mark.parametrize("active", [False, True])
def test_nan_stays_in_its_ray_and_behind_its_sample(active):
    """A NaN density at sample 70 of ray 5 (17 rays, T = 130): the ray's samples before it keep the clean run's bits, those from
    it on are NaN, as are weights_sum and depth, and none of them is in the mask or the list; every other ray is bit-equal to the
    clean run, forward and adjoint.  An inf there is alpha = 1: the float64 reference's weights."""
    N, T, C, R, S = 17, 130, 2, 5, 70
    c = rc.numeric_case(N, T, active, C)
    clean = _everything(c)
    bad = dict(c, sigma=c["sigma"].copy())
    bad["sigma"][R, S] = np.nan
    f = _everything(bad)
    others = np.arange(N) != R
    for k in ("weights", "weights_sum", "depth", "mask", "image", "d_sigma"):
        assert_bits(f[k][others], clean[k][others], k + " of the other rays")
    assert_bits(f["d_attr"].reshape(N, T, C)[others], clean["d_attr"].reshape(N, T, C)[others], "d_attr of the other rays")
    assert_bits(f["weights"][R, :S], clean["weights"][R, :S], "weights in front of the NaN")
    assert np.isnan(f["weights"][R, S:]).all() and np.isnan(f["weights_sum"][R]) and np.isnan(f["depth"][R])
    assert_bits(f["mask"][R, :S], clean["mask"][R, :S], "mask in front of the NaN")
    assert not f["mask"][R, S:].any()
    idx = check_work_list(f, N, T)  # (NaN > 1e-4 is false)
    assert not ((idx >= R * T + S) & (idx < (R + 1) * T)).any()
    assert f["count"] == clean["count"] - int(clean["mask"][R, S:].sum())
    # inf: alpha = 1, the transmittance behind it is 1e-15
    bad["sigma"][R, S] = np.inf
    f = fwd(bad)
    f64 = rc.composite_ref64(bad["sigma"], bad["z"], bad["sample_dist"], bad["density_scale"], active)
    assert np.isfinite(f64["weights"]).all() and f64["weights"][R, S] == f64["trans"][R, S]
    for k in ("weights", "weights_sum", "depth"):
        assert np.isfinite(f[k]).all()
        rc.assert_close(f[k], f64[k], *rc.TOL[k], what=k + " with an inf density")
    assert (f["weights"][R, S + 1:] <= 2e-15).all()
    assert_bits(f["weights"][others], clean["weights"][others], "weights of the other rays")
