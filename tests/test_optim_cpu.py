"""CPU tests of the references in tests/optim_cases.py, which tests/test_gpu_optim_edges.py compares the optimiser kernels with:
fp32 torch.optim.Adam stays inside the derived bounds of the float64 run with a factor two to spare, a flushed subnormal v lies
outside them, every check body passes against the float32 restatement of the kernels and fails against it with a fault switched
on.  Prints the measurements that tests/optim_cases.py records."""
import numpy as np
import pytest
import torch

import optim_cases as oc

F16, F32, F64 = np.float16, np.float32, np.float64


def _torch_f32_run(c, param0, grads):
    """fp32 torch.optim.Adam over the case, fed the gradient scaled in fp32.  -> per step (p, m, v) [total]."""
    R = len(c["lens"])
    mults = c["lr_mults"] or [1.0] * R
    P = [torch.from_numpy(param0[o:o + l].copy()).requires_grad_(True) for o, l in zip(c["offs"], c["lens"])]
    opt = torch.optim.Adam([{"params": [p], "lr": oc.LR * m} for p, m in zip(P, mults)], betas=(oc.B1, oc.B2), eps=oc.EPS)
    gs = F32(c["grad_scale"]) * (F32(1.0 / c["loss_scale"]) if c["loss_scale"] else F32(1.0))
    cur = [param0.copy(), np.zeros_like(param0), np.zeros_like(param0)]
    out = []
    for it in range(c["steps"]):
        factor = float(F32(0.1 ** min(it / c["sched"], 1.0))) if c["sched"] else 1.0
        on = oc.open_ranges(c, it)
        for r, (p, o, l) in enumerate(zip(P, c["offs"], c["lens"])):
            opt.param_groups[r]["lr"] = oc.LR * mults[r] * factor
            p.grad = torch.from_numpy(grads[it][o:o + l] * gs) if on[r] else None
        opt.step()
        cur = [a.copy() for a in cur]
        for r, (p, o, l) in enumerate(zip(P, c["offs"], c["lens"])):
            if on[r] and l:
                st = opt.state[p]
                cur[0][o:o + l], cur[1][o:o + l], cur[2][o:o + l] = p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        out.append(cur)
    return out


def test_constants_of_the_derivation():
    assert [round(v, 2) for v in (oc.DB1, oc.DB2, oc.DW2, oc.C_STEP, oc.C_RS2)] == [2.0, 0.08, 8.0, 5.0, 5.0]


def test_fp32_torch_adam_is_inside_the_bounds_with_a_factor_two():
    spare = [np.inf] * 3
    cases = [oc.ranges_case(n) for n in ("mixed", "mixed_no_scaler", "lengths")] + [oc.flat_case()]
    # the issue's own measurement: six steps at gradient magnitudes 1e-8 .. 1e6
    cases.append(dict(oc.flat_case(1025), mags=[1e-8, 1e6, 1e-3, 1.0, 1e3, 1e-6], steps=6, grad_scale=1.0))
    for c in cases:
        b, grads, inside = oc.case_arrays(c)
        ref = oc.adam_reference(c, b["param"], grads)
        run = _torch_f32_run(c, b["param"], grads)
        for it in range(c["steps"]):
            for j, (rk, ek) in enumerate((("p", "Ep"), ("m", "Em"), ("v", "Ev"))):
                half = ref[it][ek][inside] / 2
                spare[j] = min(spare[j], 2 * oc.assert_within(run[it][j][inside], ref[it][rk][inside], half, f"fp32 torch, step {it}, {rk}"))
    print(f"fp32 torch.optim.Adam against float64, smallest bound / error: parameter {spare[0]:.1f}, exp_avg {spare[1]:.1f}, exp_avg_sq {spare[2]:.1f}")
    assert min(spare) >= 2.0


def test_flushed_subnormal_v_is_outside_the_bound():
    c, b, grads, inside = oc.values_case()
    ref = oc.adam_reference(c, b["param"], grads)[0]
    for i in oc.I_SUBNORMAL:
        v32 = F32(ref["v"][i])
        assert 0 < v32 < 2.0 ** -126 and abs(float(v32) - ref["v"][i]) <= oc.S_SUB / 2     # half a subnormal ulp
        gap = abs(oc.flushed_update(c, ref, i) - ref["p"][i])
        print(f"g = {oc.VALUE_GRADS[i]:g}: update {ref['p'][i]:.3e}, bound {ref['Ep'][i]:.2e}, flushed v' is {gap:.2e} away = {gap / ref['Ep'][i]:.1f} bounds")
        assert gap > 2 * ref["Ep"][i]
    for i in oc.I_UNDERFLOW:
        assert F32(ref["v"][i]) == 0
        rounded = -oc.LR / (1 - oc.B1) * ref["m"][i] / oc.EPS        # the float64 formula on the fp32-rounded v' = 0
        assert abs(rounded - ref["p"][i]) <= 1e-12 * abs(ref["p"][i]) < ref["Ep"][i]


def test_adam_bodies_pass_against_the_restatement():
    impl = oc.Restated()
    for name in oc.RANGES_CASES:
        spare = oc.check_adam_ranges(impl, name)
        print(f"restatement, {name}: smallest bound / error: parameter {spare[0]:.1f}, exp_avg {spare[1]:.1f}, exp_avg_sq {spare[2]:.1f}")
    for n in oc.ADAM_LENGTHS:
        oc.check_adam_flat(impl, n)
    oc.check_adam_flat(impl, 1025, with_f16=False)
    oc.check_adam_values(impl)
    oc.check_adam_noops_and_skip(impl)
    oc.check_adam_refusals(impl)


@pytest.mark.parametrize("fault", ["tail_one_element", "tail_one_too_far"])
def test_a_wrong_tail_is_caught(fault):
    impl = oc.Restated(fault)
    want = "outside the bound" if fault == "tail_one_element" else "padding or guard|the guard of"
    with pytest.raises(AssertionError, match=want):
        oc.check_adam_ranges(impl, "mixed")
    with pytest.raises(AssertionError, match=want):
        oc.check_adam_ranges(impl, "lengths")
    for n in (3, 7, 1023):
        with pytest.raises(AssertionError, match=want):
            oc.check_adam_flat(impl, n)
    for n in (4, 8, 1024):        # no tail: no fault
        oc.check_adam_flat(impl, n)


def test_a_shared_step_counter_is_caught():
    impl = oc.Restated("shared_step")
    with pytest.raises(AssertionError, match="outside the bound"):
        oc.check_adam_ranges(impl, "mixed")
    oc.check_adam_ranges(impl, "mixed_ungated")     # every range open at every step: the counters agree, no fault


def test_the_other_bodies_pass_against_the_restatement():
    impl = oc.Restated()
    oc.check_cast(impl)
    for n in oc.REDUCE_SMALL:
        oc.check_nonfinite(impl, n)
        oc.check_absmax(impl, n)
    oc.check_absmax(impl, oc.ABSMAX_BIG)
    oc.check_reduce_edges(impl)
    oc.check_scaler(impl)
    oc.check_slices(impl)


def test_positions_cover_both_sweeps_and_the_tail():
    for n, cap in ((oc.NONFINITE_BIG, oc.NONFINITE_CAP), (oc.ABSMAX_BIG, oc.ABSMAX_CAP)):
        p = oc.positions(n, cap)
        assert {0, 255, 256, cap * 1024 - 1, cap * 1024, n - 4, n - 3, n - 2, n - 1} <= set(p) and n % 4 == 3
    assert oc.positions(5, 256) == [0, 3, 4] and oc.positions(3, 256) == [0, 1, 2]
