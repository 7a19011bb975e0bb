"""CPU tests of the references in tests/render_cases.py, which tests/test_gpu_render_edges.py compares the sampling and
compositing kernels with: that the float64 reference says what torch autograd and oracle/fields_ref.py say, that the structural
closed forms are what a float32 restatement of the kernels computes (and not what it computes with a wrong carry), that every
lattice is exact and every sampling case clamps on all six faces (the references assert it while they are built here), and that
every tolerance of the numeric class holds for the float32 restatement with a factor four to spare.  Prints the measurements
that tests/render_cases.py records."""
import numpy as np
import pytest
import torch

import render_cases as rc

F32, F64 = np.float32, np.float64


def _restated(c, attr, C, grads, fault=None, want_image=False):
    """Forward and adjoint of a structural case through the float32 restatement."""
    f = rc.composite_fwd_f32(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], c["active"], fault)
    ds, da = rc.composite_bwd_f32(c["sigma"], c["z"], f["weights"], attr, C, c["sample_dist"], c["density_scale"], c["active"],
                                  grads.get("d_depth"), grads.get("d_wsum"), grads.get("d_image"), grads.get("d_weights"), fault)
    return f, ds, da


# ---- sampling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", rc.SAMPLE_SHAPES)
def test_sampling_cases_clamp_on_all_six_faces(N, T):
    for with_noise in (False, True):
        cases = rc.sample_cases(N, T, with_noise)  # asserts the coverage
        assert len(cases) == 3 and [c["bound"] for c in cases] == list(rc.SAMPLE_BOUNDS)


@pytest.mark.parametrize("N,T", [(3, 85), (5, 768)])
def test_sampling_restatement_is_the_renderer_formula(N, T):
    """z_vals: bit-equal to oracle.fields_ref.sample_z in float32 (the same operations on torch's linspace); the points agree with
    the float64 evaluation of clamp(o + d z) and (x + bound) / (2 bound) to fp32 rounding."""
    from oracle import fields_ref
    lin = torch.linspace(0.0, 1.0, T).numpy()
    for c in rc.sample_cases(N, T, True):
        z, xyz, xt, _ = rc.sample_ref(c["rays_o"], c["rays_d"], lin, c["noise"], c["near"], c["far"], c["bound"])
        zt, _ = fields_ref.sample_z(N, c["near"], c["far"], T, torch.from_numpy(c["noise"]))
        assert rc.same_bits(z, zt.numpy()).all()
        b = float(F32(c["bound"]))
        p = np.clip(c["rays_o"].astype(F64)[:, None] + c["rays_d"].astype(F64)[:, None] * z.astype(F64)[:, :, None], -b, b)
        assert np.abs(xyz.reshape(N, T, 3) - p).max() <= 2.0 ** -23 * b
        assert np.abs(xt[:, :3].reshape(N, T, 3) - (p + b) / (2 * b)).max() <= 2.0 ** -23
        assert rc.same_bits(xt[:, 3], np.full(N * T, rc.SAMPLE_T, F32)).all()


# ---- the float64 reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,active,C", [(1, False, 2), (65, True, 2), (130, False, 3), (1025, True, 1)])
def test_float64_adjoint_is_autograd_of_the_float64_forward(T, active, C):
    """... and the float64 forward is oracle.fields_ref.composite evaluated in double."""
    from oracle import fields_ref
    c = rc.numeric_case(5, T, active, C)
    N = c["N"]
    sigma = torch.from_numpy(c["sigma"]).double().requires_grad_(True)
    attr = torch.from_numpy(c["attr"]).double().requires_grad_(True)
    z = torch.from_numpy(c["z"]).double()
    ds32, sd32 = float(F32(c["density_scale"])), float(F32(c["sample_dist"]))
    w = fields_ref.composite(sigma, z, torch.full((N, 1), sd32, dtype=torch.float64), ds32, active)
    depth, wsum, image = (w * z).sum(-1), w.sum(-1), (w.unsqueeze(-1) * attr.view(N, T, C)).sum(-2)
    gd, gs, gi, gw = (torch.from_numpy(c[k]).double() for k in ("d_depth", "d_wsum", "d_image", "d_weights"))
    ((depth * gd).sum() + (wsum * gs).sum() + (image * gi).sum() + (w * gw).sum()).backward()
    f = rc.composite_ref64(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], active, c["attr"], C)
    d_sigma, d_attr = rc.composite_bwd_ref64(c, f)
    # (the oracle forms alpha as 1 - exp(-x): one ulp of 1 in float64 where the reference's -expm1(-x) has none)
    for got, want, what in ((f["weights"], w, "weights"), (f["weights_sum"], wsum, "weights_sum"), (f["depth"], depth, "depth"),
                            (f["image"], image, "image"), (d_attr, attr.grad, "d_attr")):
        rc.assert_close(got, want.detach().numpy(), 1e-12, 1e-15, what)
    g = sigma.grad.numpy()
    rc.assert_close(d_sigma, g, 1e-9, 1e-13 * np.abs(g).max(), "d_sigma")


def test_float64_forward_of_nonfinite_sigma():
    c = rc.numeric_case(2, 130, False, 2)
    c["sigma"][1, 70] = np.inf
    f = rc.composite_ref64(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], False)
    assert np.isfinite(f["weights"]).all() and f["weights"][1, 70] == f["trans"][1, 70] and (f["weights"][1, 71:] < 1e-15).all()


# ---- structure ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", rc.STRUCT_SHAPES)
def test_closed_forms_are_what_the_restatement_computes(N, T):
    """Forward, image and adjoint (C = 2, every gradient present), both sensor modes; and they agree with the float64 reference up
    to the 1e-15 terms."""
    for active in (False, True):
        c = rc.struct_inputs(N, T, active)
        attr, grads = rc.struct_attr(N, T, 2), rc.struct_grads(N, T, 2)
        f, ds, da = _restated(c, attr, 2, grads)
        rc.struct_check_fwd(c, f)
        rc.struct_check_bwd(c, attr, 2, grads, ds, da)
        rc.assert_values(rc.composite_image_f32(f["weights"], attr, 2), rc.struct_image_ref(c, attr, 2), "image")
        c64 = dict(c, C=2, attr=attr, **grads)
        f64 = rc.composite_ref64(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], active, attr, 2)
        ref = rc.struct_fwd_ref(c)
        tol = 2e-15 * T  # float64 keeps the factors 1 + 1e-15 of the clear samples that fp32 rounds to 1
        assert np.abs(f64["weights"] - ref["weights"]).max() <= tol and np.abs(f64["depth"] - ref["depth"]).max() <= tol
        d64 = rc.composite_bwd_ref64(c64, f64)[0]
        assert np.abs(d64 - rc.struct_bwd_ref(c, attr, 2, grads)[0]).max() <= 1e-12


@pytest.mark.parametrize("T", [65, 1025])
def test_closed_forms_for_every_width_and_null_gradient(T):
    N = 17
    c = rc.struct_inputs(N, T, True)
    for C in (0, 1, 3, 4):
        attr = rc.struct_attr(N, T, C) if C else None
        grads = rc.struct_grads(N, T, C)
        if not C:
            grads["d_image"] = None
        f, ds, da = _restated(c, attr, C, grads)
        rc.struct_check_bwd(c, attr, C, grads, ds, da)
    attr, full = rc.struct_attr(N, T, 2), rc.struct_grads(N, T, 2)
    for drop in ("d_depth", "d_wsum", "d_image", "d_weights"):
        grads = dict(full, **{drop: None})
        f, ds, da = _restated(c, attr, 2, grads)
        rc.struct_check_bwd(c, attr, 2, grads, ds, da)
    none = dict.fromkeys(full)
    f, ds, da = _restated(c, attr, 2, none)
    rc.struct_check_bwd(c, attr, 2, none, ds, da)
    assert (ds == 0).all() and (rc.struct_bwd_ref(c, attr, 2, none)[0] == 0).all()


@pytest.mark.parametrize("T", sorted(rc.STRUCT_MULTI))
def test_closed_forms_with_two_and_three_opaque_samples(T):
    for active in (False, True):
        c = rc.struct_inputs(len(rc.STRUCT_MULTI[T]), T, active, rc.STRUCT_MULTI[T])
        f = rc.composite_fwd_f32(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], active)
        rc.struct_check_fwd(c, f)
        ref = rc.struct_fwd_ref(c)
        assert sorted(set(ref["weights"].reshape(-1).tolist())) == [0.0, float(rc.EPS_T * rc.EPS_T), float(rc.EPS_T), 1.0]


def test_closed_forms_catch_a_wrong_carry():
    """A chunk carry that leaves out the chunk's last sample fails the structural check at T = 65, a transmittance that starts
    again at 1 in every segment fails it at T = 1025: forward (two opaque samples) and adjoint (one)."""
    for T, fault, positions in ((65, "carry_shift", [(63, 64)]), (1025, "no_segment_carry", [(3, 1024), (1023, 1024)])):
        c = rc.struct_inputs(len(positions), T, False, positions)
        rc.struct_check_fwd(c, rc.composite_fwd_f32(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], False))
        with pytest.raises(AssertionError, match="weights"):
            rc.struct_check_fwd(c, rc.composite_fwd_f32(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], False, fault))
        c = rc.struct_inputs(33, T, False)
        attr, grads = rc.struct_attr(33, T, 2), rc.struct_grads(33, T, 2)
        f, ds, da = _restated(c, attr, 2, grads, fault)
        rc.struct_check_fwd(c, f)  # (one opaque sample per ray: the forward does not see the carry)
        with pytest.raises(AssertionError, match="d_sigma"):
            rc.struct_check_bwd(c, attr, 2, grads, ds, da)
        other = "no_segment_carry" if fault == "carry_shift" else "carry_shift"
        if T == 65:  # one segment: the other fault is no fault here
            f, ds, da = _restated(c, attr, 2, grads, other)
            rc.struct_check_bwd(c, attr, 2, grads, ds, da)


# ---- numerics -------------------------------------------------------------------------------------------------------------------
def test_restatement_meets_every_tolerance_with_a_factor_four():
    """The float32 restatement against float64 over NUMERIC_CASES: its excess over the rtol term stays within a quarter of every
    atol, four times its d_sigma excess is within DSIGMA_K, and the borderline samples of the mask stay below 1 % of the kept."""
    worst = dict.fromkeys(list(rc.TOL) + ["d_sigma"], -np.inf)
    worst_borderline, alpha_max = (0, 1), 0.0
    for N, T, active, C in rc.NUMERIC_CASES:
        c = rc.numeric_case(N, T, active, C)
        f64 = rc.composite_ref64(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], active, c["attr"], C)
        ds64, da64 = rc.composite_bwd_ref64(c, f64)
        f32 = rc.composite_fwd_f32(c["sigma"], c["z"], c["sample_dist"], c["density_scale"], active)
        f32["image"] = rc.composite_image_f32(f32["weights"], c["attr"], C)
        ds32, da32 = rc.composite_bwd_f32(c["sigma"], c["z"], f32["weights"], c["attr"], C, c["sample_dist"], c["density_scale"], active,
                                          c["d_depth"], c["d_wsum"], c["d_image"], c["d_weights"])
        for k, got, ref in [(k, f32[k], f64[k]) for k in ("weights", "weights_sum", "depth", "image")] + [("d_attr", da32, da64)]:
            e = rc.excess(got, ref, rc.TOL[k][0])
            worst[k] = max(worst[k], e)
            assert e <= rc.TOL[k][1] / 4, (k, N, T, active, C, e)
        e = rc.excess(ds32, ds64, rc.DSIGMA_RTOL) / np.abs(ds64).max()
        worst["d_sigma"] = max(worst["d_sigma"], e)
        assert 4 * e <= rc.DSIGMA_K, (N, T, active, C, e)
        kept, bl = int((f64["weights"] > float(rc.MASK_THRESHOLD)).sum()), int(rc.borderline(f64["weights"]).sum())
        diff = (f32["mask"] != (f64["weights"] > float(rc.MASK_THRESHOLD))) & ~rc.borderline(f64["weights"])
        assert not diff.any(), "the restatement's mask differs from the reference away from the threshold"
        assert bl < rc.BORDERLINE_CAP * kept, (N, T, active, C, bl, kept)
        if bl * worst_borderline[1] >= worst_borderline[0] * max(kept, 1):
            worst_borderline = (bl, max(kept, 1))
        alpha_max = max(alpha_max, float(1.0 - (f64["fac"] - float(rc.EPS_T)).min()))
        assert np.isfinite(ds64).all() and (c["z"][:, 1:] > c["z"][:, :-1]).all()
    print("float32 restatement against float64, largest excess over the rtol term:")
    for k, v in worst.items():
        print(f"    {k:12s} {v:+.2e}" + ("  (relative to max|ref d_sigma|; DSIGMA_K needs >= %.2e)" % (4 * v) if k == "d_sigma" else ""))
    print(f"    borderline mask samples: at most {worst_borderline[0]} of {worst_borderline[1]} kept; largest alpha {alpha_max:.7f}")
    # (T = 1 and 2 have the long intervals: 1 - alpha goes down to 3e-6 there, still 50 fp32 ulps of 1)
    assert alpha_max > 0.9 and 1.0 - alpha_max > 1e-6, "the inputs should reach a large alpha without saturating it in fp32"


def test_numeric_rays_do_not_depend_on_the_batch():
    big = rc.numeric_case(33, 1025, False, 2)
    one = rc.numeric_case(1, 1025, False, 2)
    sub = rc.take_rays(big, [0, 15, 16, 32])
    assert sub["N"] == 4 and sub["attr"].shape == (4 * 1025, 2)
    for k in ("z", "sigma", "attr", "d_depth", "d_wsum", "d_image", "d_weights"):
        assert rc.same_bits(rc.take_rays(big, [0])[k], one[k]).all(), k
    assert rc.same_bits(sub["sigma"][3], big["sigma"][32]).all()
