"""Inputs, references and check bodies for the edge tests of the optimiser kernels (tests/test_optim_cpu.py,
tests/test_gpu_optim_edges.py): adam_kernel, adam_advance_kernel / adam_ranges_kernel, cast_kernel, nonfinite_check_kernel,
absmax_kernel, scaler_update_kernel and mark_slices_kernel of csrc/optim.hip.  Nothing here is computed by HIP code.

Every check body (``check_*``) takes an implementation object with one method per C entry point; a method gets the entry point's
buffers as numpy arrays (prefilled by the body, changed in place) and its scalar arguments, and returns None or the refusal's
message.  The device tests pass ``ops.call`` wrapped that way; tests/test_optim_cpu.py passes ``Restated``, a float32 numpy
restatement of the kernels, first as it is (every body passes) and then with a fault (the body fails): tail_one_element (the scalar
tail handles one element), tail_one_too_far (it runs one element past the range), shared_step (one step counter for all ranges).

Adam: the reference and its bounds
----------------------------------
The reference is torch.optim.Adam on the CPU in float64, betas (0.9, 0.99), eps 1e-15, one parameter tensor per range, fed the fp32
gradients multiplied in float64 by grad_scale and 1 / loss scale; ``.grad = None`` stands for a closed gate, so every range has its
own step count.  The bounds are a running first-order error analysis of the kernel's fp32 operations, evaluated per element next to
the reference (``adam_reference``).  u = 2^-23, one ulp: every fp32 operation is allowed faithful rounding (an error of up to one
ulp, u relative), twice what round-to-nearest does -- a build without correctly rounded division and square root would still be
inside, and it is where the factor two comes from that fp32 torch.optim.Adam, which rounds to nearest, keeps to these bounds.
s = 2^-149, a rounding that lands in the subnormals.  The deviations of the constants are what they are, not doubled:
  g   = grad * (grad_scale * scaler[3]): two roundings, 2 u |g|.
  m'  = m + (g - m) * (1 - b1).  b1 arrives as a float: 1 - (float)0.9 is 2.0 u above 0.1 (DB1).  The difference, the product and
        the sum round:  E_m' = b1 E_m + u [(1 - b1) (2 |g| + (2 + DB1) |g - m|) + |m'|] + s.
  v'  = v * b2 + (1 - b2) * g * g.  (float)0.99 is 0.08 u above 0.99 (DB2), 1 - (float)0.99 is 8.0 u below 0.01 (DW2); v * b2
        rounds, the contribution has g twice (4 u) and two products (2 u), the sum rounds:
        E_v' = b2 E_v + u [(DB2 + 1) b2 v + (DW2 + 6) (1 - b2) g^2 + v'] + 2 s.
  step = lr / bias_c1: the rate as a float, the schedule's factor as a float, bias_c1 from (float)0.9 (at t = 1 it is 1 - b1: DB1),
        the result rounded: C_STEP = 3 + DB1 = 5 u relative.
  rs2 = sqrt(bias_c2): bias_c2 from (float)0.99 (DW2 at t = 1, less later), half of it through the root, one rounding:
        C_RS2 = DW2 / 2 + 1 = 5 u.
  denom = sqrt(v') / rs2 + eps: d sqrt(v') <= min(E_v' / (2 sqrt v'), sqrt(E_v')) (the second when v' underflows); sqrtf, the
        division and the sum round:  E_d = d sqrt(v') / rs2 + (sqrt(v') / rs2) (C_RS2 + 2) u + u denom.
  q = m' / denom:  E_q = E_m' / denom + |q| E_d / denom + u |q|.      upd = step * q:  E_u = step E_q + (C_STEP + 1) u |upd|.
  p' = p - upd:  E_p' = E_p + E_u + u |p'| + s.
"A few ulps of max(|old|, |contribution|)" for the moments (2.2 u and 16 u of it per step at the most), "ulps of |p| plus ulps of
the step" for the parameter.  Nothing in them comes from a kernel's output.

Measured on the CPU (tests/test_optim_cpu.py prints it): the smallest ratio bound / error over all elements and steps of the cases
below and of six steps at gradient magnitudes 1e-8 .. 1e6,
    fp32 torch.optim.Adam (double betas, round to nearest; the test requires 2):   parameter 2.2   exp_avg 6.8   exp_avg_sq 11.7
    the restatement of the kernels (float betas; must be inside):                  parameter 2.2   exp_avg 2.3   exp_avg_sq 1.6
    MI355X, the kernels (tests/test_gpu_optim_edges.py prints it):                 parameter 2.2   exp_avg 2.3   exp_avg_sq 1.6
(the parameter's 2.2 is one subtraction rounding by half an ulp of a parameter just above a power of two; the restatement's 1.6
is DW2, a deviation with a fixed sign.)
Subnormal v (g = 1e-20 from zero moments: v' = 1e-42, 714 subnormal ulps, known to half a subnormal ulp): the bound on the
parameter is 1.92e-13 at an update of 1.0e-7 (E_v' = 2 s moves denom by 1.4e-24, far below u denom); a kernel that flushed v' to
zero would have denom = eps instead of eps + 1e-20 and an update 1.0e-12 away, 5.2 times the bound -- the CPU test asserts that
separation, the device test the bound.
v' that underflows (g = 1e-30): the float64 reference with v' rounded to fp32 (zero) is 1e-15 relative from the reference itself.

Observed behaviour of l4d_scaler_update, recorded and not judged: the scale is an fp32 product, so backing off from 2^-126 walks
through the subnormals (2^-127 with 1 / scale = 2^127, then 2^-128 with 1 / scale = +inf), and growing past 2^127 gives +inf with
1 / scale = 0.  Both are what the float64 rule rounded to fp32 gives.
l4d_mark_time_slices with t outside [0, 1] marks slice -1 or n_slices like common.h slice_pair says: the bodies hand the kernel a
gate array with sentinel floats on both sides, so those stores land in the test's own buffer.
"""
import numpy as np
import torch

from glue_cases import F16, F32, F64, rng_of, same_bits  # noqa: F401

U, S_SUB = 2.0 ** -23, 2.0 ** -149
B1, B2, EPS = 0.9, 0.99, 1e-15
B1F, B2F = float(F32(B1)), float(F32(B2))
DB1 = abs((1.0 - B1F) - (1.0 - B1)) / (1.0 - B1) / U          # 2.0
DB2 = abs(B2F - B2) / B2 / U                                    # 0.08
DW2 = abs((1.0 - B2F) - (1.0 - B2)) / (1.0 - B2) / U          # 8.0
C_STEP, C_RS2 = 3.0 + DB1, DW2 / 2.0 + 1.0
FLT_MAX = F32(3.4028235e38)
SENT_P, SENT_M, SENT_V, SENT_G, SENT_H = F32(-12345.0), F32(-23456.0), F32(34567.0), F32(-45678.0), F16(-77.0)
GUARD = 8
MAX_RANGES = 40
MSG = dict(many="l4d_adam_step_ranges: too many ranges", off="l4d_adam_step_ranges: range offsets must be multiples of 4 elements",
           gate="l4d_adam_step_ranges: gated range without a gate buffer",
           align_r="l4d_adam_step_ranges: buffers must be 16-byte aligned (fp16 copy 8-byte)",
           align="l4d_adam_step: buffers must be 16-byte aligned (fp16 copy 8-byte)",
           cast="l4d_cast: src must be 16-byte, dst 8-byte aligned", nonfinite="l4d_grad_nonfinite_check: grad must be 16-byte aligned",
           absmax="l4d_absmax_f32: x must be 16-byte aligned")
ADAM_BUFFERS = ("param", "grad", "exp_avg", "exp_avg_sq", "param_f16")
FAULTS = (None, "tail_one_element", "tail_one_too_far", "shared_step")


# =================================================================================================================================
# the float32 restatement
# =================================================================================================================================
def _adam_elements(b, idx, step, rs2, gs, b1, b2, eps, with_f16):
    with np.errstate(all="ignore"):
        g = b["grad"][idx] * gs
        m = b["exp_avg"][idx]
        m = m + (g - m) * (F32(1.0) - b1)
        v = b["exp_avg_sq"][idx] * b2 + (F32(1.0) - b2) * g * g
        denom = np.sqrt(v) / rs2 + eps
        p = b["param"][idx] - step * (m / denom)
    assert p.dtype == m.dtype == v.dtype == F32
    b["param"][idx], b["exp_avg"][idx], b["exp_avg_sq"][idx] = p, m, v
    if with_f16:
        with np.errstate(all="ignore"):
            b["param_f16"][idx] = p.astype(F16)


def _body_and_tail(off, n, fault):
    """Element indices one launch touches for a range: the float4 body and the scalar tail."""
    nb = n // 4 * 4
    tail_end = n
    if fault == "tail_one_element":
        tail_end = min(nb + 1, n)
    elif fault == "tail_one_too_far" and n % 4:
        tail_end = n + 1
    return off + np.concatenate([np.arange(nb), np.arange(nb, tail_end)]).astype(np.int64)


class Restated:
    """The entry points of csrc/optim.hip in numpy float32, host checks included, in the kernels' order of operations."""

    def __init__(self, fault=None):
        assert fault in FAULTS
        self.fault = fault

    def adam_step(self, b, n, lr, b1, b2, eps, bias_c1, bias_c2, grad_scale, misalign=None):
        if n == 0:
            return None
        if misalign:
            return MSG["align"]
        step, rs2 = F32(lr) / F32(bias_c1), np.sqrt(F32(bias_c2))
        _adam_elements(b, _body_and_tail(0, n, self.fault), step, rs2, F32(grad_scale), F32(b1), F32(b2), F32(eps), b["param_f16"] is not None)
        return None

    def adam_step_ranges(self, b, n_ranges, off, ln, lr, gate_idx, b1, b2, eps, grad_scale, sched_iters, misalign=None):
        """b: param, grad, exp_avg, exp_avg_sq, param_f16 | None, gates | None, scaler | None, steps, sched | None."""
        if n_ranges == 0:
            return None
        if n_ranges > MAX_RANGES:
            return MSG["many"]
        for r in range(n_ranges):
            if off[r] & 3:
                return MSG["off"]
            if gate_idx is not None and gate_idx[r] >= 0 and b["gates"] is None:
                return MSG["gate"]
        if misalign:
            return MSG["align_r"]
        if max(ln[:n_ranges]) == 0:
            return None
        scaler, gates, sched = b["scaler"], b["gates"], b["sched"]
        skip = scaler is not None and scaler[2] != 0
        on = [not skip and (gate_idx is None or gate_idx[r] < 0 or gates[gate_idx[r]] != 0) for r in range(n_ranges)]
        for r in range(n_ranges):
            if on[r]:
                b["steps"][r] += 1
        if sched is not None:
            it = float(sched[0])
            sched[1] = F32(0.1 ** min(it / float(F32(sched_iters)), 1.0))
            sched[0] = F32(it + 1.0)
        b1, b2, eps = F32(b1), F32(b2), F32(eps)
        gs = F32(grad_scale) * (scaler[3] if scaler is not None else F32(1.0))
        for r in range(n_ranges):
            if not on[r] or ln[r] == 0:
                continue
            t = float(b["steps"][0 if self.fault == "shared_step" else r])
            rate = float(F32(lr[r])) * (float(sched[1]) if sched is not None else 1.0)
            with np.errstate(all="ignore"):
                step = F32(rate / (1.0 - float(b1) ** t))
                rs2 = F32(np.sqrt(1.0 - float(b2) ** t))
            _adam_elements(b, _body_and_tail(off[r], ln[r], self.fault), step, rs2, gs, b1, b2, eps, b["param_f16"] is not None)
        return None

    def cast(self, src, dst, n, misalign=None):
        if n == 0:
            return None
        if misalign:
            return MSG["cast"]
        with np.errstate(all="ignore"):
            dst[:n] = src[:n].astype(F16)
        return None

    def nonfinite(self, x, pokes, n, state, misalign=False):
        if n == 0:
            return None
        if misalign:
            return MSG["nonfinite"]
        x = _poked(x, pokes)[:n]
        if (~(np.abs(x) <= FLT_MAX)).any():
            state[2] = F32(1.0)
        return None

    def absmax(self, x, pokes, n, out, misalign=False):
        out[0] = F32(0.0)
        if n == 0:
            return None
        if misalign:
            return MSG["absmax"]
        x = _poked(x, pokes)[:n]
        out[0] = F32(np.inf) if (~(np.abs(x) <= FLT_MAX)).any() else np.abs(x).max()
        return None

    def scaler_update(self, state, growth, backoff, interval):
        with np.errstate(all="ignore"):
            if state[2] != 0:
                state[0] = state[0] * F32(backoff)
                state[1] = F32(0.0)
            else:
                state[1] = state[1] + F32(1.0)
                if state[1] >= F32(interval):
                    state[0] = state[0] * F32(growth)
                    state[1] = F32(0.0)
            state[2] = F32(0.0)
            state[3] = F32(1.0) / state[0]
        return None

    def mark_time_slices(self, t, n_slices, gates, base):
        """gates: the whole buffer, slice 0 at index ``base``."""
        from hashgrid_cases import slice_pair_f32
        i1, i2, _, _ = slice_pair_f32(t, n_slices)
        gates[base + i1] = gates[base + i2] = F32(1.0)
        return None


def _poked(x, pokes):
    if not pokes:
        return x
    x = x.copy()
    for i, v in pokes:
        x[i] = v
    return x


# =================================================================================================================================
# Adam: cases, reference, bodies
# =================================================================================================================================
def pad4(n):
    return (n + 3) // 4 * 4


def layout(lens):
    """Offsets padded to 4 elements (the documented requirement) and the arena's length without the guard."""
    offs, o = [], 0
    for n in lens:
        offs.append(o)
        o += pad4(n)
    return offs, o


ADAM_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1024 * 4 + 3)
LR = 1e-2


def ranges_case(name):
    """-> dict: lens, offs, total, lr_mults, gate_idx | None, n_gates, gate_steps [steps][n_gates], mags [steps], grad_scale,
    loss_scale | None (scaler state [S, 0, 0, 1 / S]), f16, sched (iters | None)."""
    c = dict(name=name, lr_mults=None, gate_idx=None, n_gates=0, gate_steps=None, grad_scale=1.0, loss_scale=None, f16=True, sched=None)
    if name.startswith("mixed"):
        # a long range beside short ones: most workgroups of the short rows must exit; the zero-length range shares gate 0
        c.update(lens=[1, 3, 4, 5, 1025, 0], lr_mults=[1.0, 1.0, 0.1, 0.1, 1.0, 1.0], gate_idx=[-1, 0, 1, 1, 2, 0], n_gates=3,
                 gate_steps=[(1, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1)], mags=[1e-2, 1e3, 1e-5, 1.0, 1e6],
                 grad_scale=0.25, loss_scale=8.0, sched=4.0)
        if name == "mixed_no_f16":
            c["f16"] = False
        elif name == "mixed_no_scaler":
            c["loss_scale"] = None
        elif name == "mixed_ungated":
            c.update(gate_idx=[-1] * 6, n_gates=0, gate_steps=None)
        else:
            assert name == "mixed"
    elif name == "lengths":
        c.update(lens=[2, 7, 8, 1023, 1024, 1024 * 4 + 3], lr_mults=[1.0, 0.1, 1.0, 0.1, 1.0, 1.0], mags=[1e-8, 1e2, 1e-3], sched=2.0)
    else:
        raise KeyError(name)
    c["offs"], c["total"] = layout(c["lens"])
    c["steps"] = len(c["mags"])
    return c


RANGES_CASES = ("mixed", "mixed_no_f16", "mixed_no_scaler", "mixed_ungated", "lengths")


def case_arrays(c):
    """Initial buffers (padding and guard hold sentinels) and the per-step gradient arenas (fp32, padding = SENT_G)."""
    total, n = c["total"], c["total"] + GUARD
    r = rng_of(41, total, len(c["lens"]))
    inside = np.zeros(n, bool)
    for o, l in zip(c["offs"], c["lens"]):
        inside[o:o + l] = True
    param = np.where(inside, r.normal(size=n) * np.exp(r.uniform(-6, 2, size=n)), SENT_P).astype(F32)
    b = dict(param=param, exp_avg=np.where(inside, 0.0, SENT_M).astype(F32), exp_avg_sq=np.where(inside, 0.0, SENT_V).astype(F32),
             param_f16=np.full(n, SENT_H, F16) if c["f16"] else None,
             gates=np.zeros(c["n_gates"] + 1, F32) if c["n_gates"] else None,
             scaler=np.array([c["loss_scale"], 5.0, 0.0, 1.0 / c["loss_scale"]], F32) if c["loss_scale"] else None,
             steps=np.concatenate([np.zeros(len(c["lens"]), np.int32), [-7]]).astype(np.int32),
             sched=np.array([0.0, 1.0, SENT_P], F32) if c["sched"] else None)
    grads = []
    for mag in c["mags"]:
        g = r.normal(size=n) * mag * (c["loss_scale"] or 1.0) / c["grad_scale"]
        grads.append(np.where(inside, g, SENT_G).astype(F32))
    return b, grads, inside


def open_ranges(c, it):
    gi = c["gate_idx"] or [-1] * len(c["lens"])
    return [g < 0 or bool(c["gate_steps"][it][g]) for g in gi]


def adam_reference(c, param0, grads, lr=LR, flat_steps=None):
    """torch.optim.Adam in float64 with the error bounds of the module docstring.  -> per step: dict(p, m, v, Ep, Em, Ev
    [total] float64, steps [ranges], factor)."""
    R = len(c["lens"])
    mults = c["lr_mults"] or [1.0] * R
    P = [torch.from_numpy(param0[o:o + l].astype(F64)).requires_grad_(True) for o, l in zip(c["offs"], c["lens"])]
    opt = torch.optim.Adam([{"params": [p], "lr": lr * m} for p, m in zip(P, mults)], betas=(B1, B2), eps=EPS)
    n = param0.size
    cur = dict(p=param0.astype(F64), m=np.zeros(n), v=np.zeros(n), Ep=np.zeros(n), Em=np.zeros(n), Ev=np.zeros(n))
    steps, out = [0] * R, []
    inv = 1.0 / c["loss_scale"] if c["loss_scale"] else 1.0
    for it in range(c["steps"]):
        factor = float(F32(0.1 ** min(it / c["sched"], 1.0))) if c["sched"] else 1.0
        on = open_ranges(c, it)
        g64 = grads[it].astype(F64) * (c["grad_scale"] * inv)
        for r, (p, o, l) in enumerate(zip(P, c["offs"], c["lens"])):
            opt.param_groups[r]["lr"] = lr * mults[r] * factor
            p.grad = torch.from_numpy(g64[o:o + l].copy()) if on[r] else None
        opt.step()
        new = {k: a.copy() for k, a in cur.items()}
        for r, (p, o, l) in enumerate(zip(P, c["offs"], c["lens"])):
            if not on[r]:
                continue
            steps[r] += 1
            if l == 0:
                continue
            st = opt.state[p]
            assert int(st["step"]) == steps[r]
            s = slice(o, o + l)
            m0, v0, g = cur["m"][s], cur["v"][s], g64[s]
            m1, v1, p1 = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy(), p.detach().numpy().copy()
            Em = B1 * cur["Em"][s] + U * ((1 - B1) * (2 * np.abs(g) + (2 + DB1) * np.abs(g - m0)) + np.abs(m1)) + S_SUB
            Ev = B2 * cur["Ev"][s] + U * ((DB2 + 1) * B2 * v0 + (DW2 + 6) * (1 - B2) * g * g + v1) + 2 * S_SUB
            t = steps[r]
            step, rs2 = lr * mults[r] * factor / (1 - B1 ** t), np.sqrt(1 - B2 ** t)
            root = np.sqrt(v1)
            with np.errstate(all="ignore"):
                d_root = np.minimum(np.where(root > 0, Ev / (2 * root), np.inf), np.sqrt(Ev))
            denom = root / rs2 + EPS
            Ed = d_root / rs2 + root / rs2 * (C_RS2 + 2) * U + U * denom
            q = m1 / denom
            Eq = Em / denom + np.abs(q) * Ed / denom + U * np.abs(q)
            Eu = step * Eq + (C_STEP + 1) * U * np.abs(step * q)
            Ep = cur["Ep"][s] + Eu + U * np.abs(p1) + S_SUB
            new["p"][s], new["m"][s], new["v"][s], new["Ep"][s], new["Em"][s], new["Ev"][s] = p1, m1, v1, Ep, Em, Ev
        cur = new
        out.append(dict(cur, steps=list(steps), factor=factor, on=on))
    return out


def assert_within(got, ref, bound, what):
    err = np.abs(np.asarray(got, F64) - ref)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (f"{what}: {bad.size} of {err.size} outside the bound, first at {bad[:4]}: got {np.asarray(got)[bad[:4]]}, "
                           f"reference {ref[bad[:4]]}, bound {bound[bad[:4]]}")
    with np.errstate(all="ignore"):
        return float(np.nanmin(np.where(err > 0, bound / err, np.inf))) if err.size else np.inf


def _copy(b):
    return {k: None if v is None else v.copy() for k, v in b.items()}


def _assert_unchanged(b, before, keys, what):
    for k in keys:
        if before[k] is None:
            assert b[k] is None
            continue
        assert same_bits(b[k], before[k]).all() if before[k].dtype.kind == "f" else (b[k] == before[k]).all(), f"{what}: {k} changed"


ALL_KEYS = ("param", "grad", "exp_avg", "exp_avg_sq", "param_f16", "gates", "scaler", "steps", "sched")


def check_adam_ranges(impl, name):
    """Several steps of one layout against the float64 reference: open ranges inside the bounds with their own step counts, the
    fp16 copy the rounding of the kernel's own fp32 result, closed ranges / padding / guard / gradient / gates / scaler
    bit-unchanged, the counters and the schedule exact.  -> smallest bound / error ratios (p, m, v)."""
    c = ranges_case(name)
    b, grads, inside = case_arrays(c)
    ref = adam_reference(c, b["param"], grads)
    R = len(c["lens"])
    lrs = [LR * m for m in c["lr_mults"]]
    spare = [np.inf] * 3
    for it in range(c["steps"]):
        b["grad"] = grads[it].copy()
        if b["gates"] is not None:
            b["gates"][:c["n_gates"]] = np.array(c["gate_steps"][it], F32) * F32(1 + it)   # any non-zero value opens a gate
            b["gates"][c["n_gates"]] = SENT_G
        before = _copy(b)
        msg = impl.adam_step_ranges(b, R, c["offs"], c["lens"], lrs, c["gate_idx"], B1, B2, EPS, c["grad_scale"], c["sched"] or 1.0)
        assert msg is None, msg
        what = f"{name} step {it}"
        _assert_unchanged(b, before, ("grad", "gates", "scaler"), what)
        for k in ("param", "exp_avg", "exp_avg_sq", "param_f16"):
            if b[k] is not None:
                assert same_bits(b[k][~inside], before[k][~inside]).all(), f"{what}: padding or guard of {k} was written"
        assert b["steps"].tolist() == ref[it]["steps"] + [-7], f"{what}: step counters {b['steps'].tolist()} != {ref[it]['steps']}"
        if c["sched"]:
            assert same_bits(b["sched"], np.array([it + 1.0, ref[it]["factor"], SENT_P], F32)).all(), f"{what}: sched {b['sched']}"
        for r, (o, l) in enumerate(zip(c["offs"], c["lens"])):
            s = slice(o, o + l)
            if not ref[it]["on"][r]:
                for k in ("param", "exp_avg", "exp_avg_sq", "param_f16"):
                    assert b[k] is None or same_bits(b[k][s], before[k][s]).all(), f"{what}: closed range {r}: {k} changed"
                continue
            for j, (k, rk, ek) in enumerate((("param", "p", "Ep"), ("exp_avg", "m", "Em"), ("exp_avg_sq", "v", "Ev"))):
                spare[j] = min(spare[j], assert_within(b[k][s], ref[it][rk][s], ref[it][ek][s], f"{what}: range {r} (length {l}) {k}"))
            if b["param_f16"] is not None:
                assert same_bits(b["param_f16"][s], b["param"][s].astype(F16)).all(), f"{what}: range {r}: fp16 copy != half(param)"
    return spare


def flat_case(n_max=ADAM_LENGTHS[-1]):
    c = dict(lens=[n_max], offs=[0], total=n_max, lr_mults=[1.0], gate_idx=None, n_gates=0, gate_steps=None, mags=[1e-3, 1e2, 1e-6],
             grad_scale=0.25, loss_scale=None, f16=True, sched=None, steps=3)
    return c


_FLAT = {}


def flat_reference():
    """Shared by every length: Adam is elementwise, so length n is the first n elements."""
    if not _FLAT:
        c = flat_case()
        b, grads, _ = case_arrays(c)
        _FLAT.update(c=c, b=b, grads=grads, ref=adam_reference(c, b["param"], grads))
    return _FLAT["c"], _copy(_FLAT["b"]), _FLAT["grads"], _FLAT["ref"]


def check_adam_flat(impl, n, with_f16=True):
    """l4d_adam_step at length n with a guard behind every buffer, three steps, grad_scale 0.25."""
    c, b0, grads, ref = flat_reference()
    m = n + GUARD
    b = dict(param=np.concatenate([b0["param"][:n], np.full(GUARD, SENT_P, F32)]), exp_avg=np.concatenate([np.zeros(n, F32), np.full(GUARD, SENT_M, F32)]),
             exp_avg_sq=np.concatenate([np.zeros(n, F32), np.full(GUARD, SENT_V, F32)]), param_f16=np.full(m, SENT_H, F16) if with_f16 else None)
    spare = [np.inf] * 3
    for it in range(c["steps"]):
        b["grad"] = np.concatenate([grads[it][:n], np.full(GUARD, SENT_G, F32)])
        before = _copy(b)
        t = it + 1
        msg = impl.adam_step(b, n, LR, B1, B2, EPS, 1.0 - B1 ** t, 1.0 - B2 ** t, c["grad_scale"])
        assert msg is None, msg
        what = f"flat n={n} step {it}"
        _assert_unchanged(b, before, ("grad",), what)
        for k in ("param", "exp_avg", "exp_avg_sq", "param_f16"):
            assert b[k] is None or same_bits(b[k][n:], before[k][n:]).all(), f"{what}: the guard of {k} was written"
        for j, (k, rk, ek) in enumerate((("param", "p", "Ep"), ("exp_avg", "m", "Em"), ("exp_avg_sq", "v", "Ev"))):
            spare[j] = min(spare[j], assert_within(b[k][:n], ref[it][rk][:n], ref[it][ek][:n], f"{what}: {k}"))
        if with_f16:
            assert same_bits(b["param_f16"][:n], b["param"][:n].astype(F16)).all(), f"{what}: fp16 copy != half(param)"
    return spare


# ---- gradient values ------------------------------------------------------------------------------------------------------------
VALUE_LENS = [8, 3]
VALUE_GRADS = {0: 0.0, 1: 1e-30, 2: 1e-20, 3: -1e-20, 4: 1.0, 5: -0.0, 6: -1e-30, 7: 3e-3, 8: 1e-20, 9: 0.0, 10: 1e-30}   # flat index -> g
I_ZERO, I_UNDERFLOW, I_SUBNORMAL = (0, 5, 9), (1, 6, 10), (2, 3, 8)


def values_case():
    c = dict(lens=VALUE_LENS, lr_mults=[1.0, 1.0], gate_idx=None, n_gates=0, gate_steps=None, mags=[1.0], grad_scale=1.0, loss_scale=None,
             f16=True, sched=None, steps=1)
    c["offs"], c["total"] = layout(c["lens"])
    b, _, inside = case_arrays(c)
    g = np.full(c["total"] + GUARD, SENT_G, F32)
    for i, v in VALUE_GRADS.items():
        g[i] = v
    small = list(I_UNDERFLOW + I_SUBNORMAL)
    b["param"][small] = 0.0   # an update of 1e-7 or 1e-17 is visible only beside a parameter of that size
    return c, b, [g], inside


def flushed_update(c, ref, i, lr=LR):
    """The parameter element i would have after the step if v' were flushed to zero (denom = eps), in float64."""
    return -lr / (1 - B1) * ref["m"][i] / EPS


def check_adam_values(impl):
    """One step from zero moments with g = 0 (parameter bit-unchanged, moments +-0), g = 1e-30 (v' underflows), g = 1e-20 (v'
    subnormal: the bound excludes a flushed v'), in a float4 body and in a tail.  Then +inf, -inf, NaN in one element each with
    the skip flag down: that element's parameter and moments turn non-finite, every other element keeps the clean run's bits."""
    c, b, grads, inside = values_case()
    ref = adam_reference(c, b["param"], grads)[0]
    b["grad"] = grads[0].copy()
    clean0 = _copy(b)
    args = (2, c["offs"], c["lens"], [LR, LR], None, B1, B2, EPS, 1.0, 1.0)
    assert impl.adam_step_ranges(b, *args) is None
    for k, rk, ek in (("param", "p", "Ep"), ("exp_avg", "m", "Em"), ("exp_avg_sq", "v", "Ev")):
        assert_within(b[k][inside], ref[rk][inside], ref[ek][inside], "gradient values: " + k)
    for i in I_ZERO:
        assert same_bits(b["param"][i:i + 1], clean0["param"][i:i + 1]).all() and b["exp_avg"][i] == 0 and b["exp_avg_sq"][i] == 0
    for i in I_UNDERFLOW:
        assert b["exp_avg_sq"][i] == 0 and b["exp_avg"][i] != 0 and np.isfinite(b["param"][i]) and b["param"][i] != 0
    for i in I_SUBNORMAL:
        assert 0 < b["exp_avg_sq"][i] < 2.0 ** -126, "v' of g = 1e-20 must be a subnormal, not zero"
    assert same_bits(b["param_f16"][inside], b["param"][inside].astype(F16)).all()
    clean = _copy(b)
    for bad_at, value in ((4, np.inf), (7, -np.inf), (9, np.nan), (0, np.nan)):
        nb = _copy(clean0)
        nb["grad"][bad_at] = value
        assert impl.adam_step_ranges(nb, *args) is None
        others = np.arange(nb["param"].size) != bad_at
        for k in ("param", "exp_avg", "exp_avg_sq", "param_f16"):
            assert same_bits(nb[k][others], clean[k][others]).all(), f"g = {value} at {bad_at}: another element's {k} changed"
            assert not np.isfinite(np.float64(nb[k][bad_at])), f"g = {value} at {bad_at}: {k} stayed finite"
    return ref


# ---- nothing to do, skipping, refusing --------------------------------------------------------------------------------------------
def check_adam_noops_and_skip(impl):
    c = ranges_case("mixed")
    b, grads, inside = case_arrays(c)
    b["grad"] = grads[0].copy()
    b["gates"][:] = 1.0
    R = len(c["lens"])
    lrs = [LR * m for m in c["lr_mults"]]
    tail = (B1, B2, EPS, c["grad_scale"], c["sched"])
    before = _copy(b)
    assert impl.adam_step_ranges(b, 0, c["offs"], c["lens"], lrs, c["gate_idx"], *tail) is None
    _assert_unchanged(b, before, ALL_KEYS, "n_ranges = 0")
    assert impl.adam_step_ranges(b, R, c["offs"], [0] * R, lrs, c["gate_idx"], *tail) is None
    _assert_unchanged(b, before, ALL_KEYS, "all lengths 0")
    # the skip flag: the schedule advances (the reference steps its LambdaLR on skipped iterations too), no step counter does
    b["scaler"][2] = 1.0
    before = _copy(b)
    assert impl.adam_step_ranges(b, R, c["offs"], c["lens"], lrs, c["gate_idx"], *tail) is None
    _assert_unchanged(b, before, ALL_KEYS[:-1], "skip flag raised")
    assert same_bits(b["sched"], np.array([1.0, 1.0, SENT_P], F32)).all(), b["sched"]
    assert impl.adam_step_ranges(b, R, c["offs"], c["lens"], lrs, c["gate_idx"], *tail) is None
    _assert_unchanged(b, before, ALL_KEYS[:-1], "skip flag raised, second call")
    assert same_bits(b["sched"], np.array([2.0, F32(0.1 ** 0.25), SENT_P], F32)).all(), b["sched"]


def check_adam_refusals(impl):
    """41 ranges, an offset of 2, a gated range without gates, each buffer one element off its alignment (both entry points):
    the documented message, and every buffer, the counters and the schedule bit-unchanged."""
    c = ranges_case("mixed")
    b, grads, inside = case_arrays(c)
    b["grad"] = grads[0].copy()
    b["gates"][:] = 1.0
    R = len(c["lens"])
    lrs = [LR * m for m in c["lr_mults"]]
    tail = (B1, B2, EPS, c["grad_scale"], c["sched"])
    before = _copy(b)

    def refused(msg, want, what):
        assert msg is not None and want in msg, f"{what}: expected a refusal with '{want}', got {msg!r}"
        _assert_unchanged(b, before, ALL_KEYS, what)

    many = MAX_RANGES + 1
    b41 = dict(b, steps=np.zeros(many + 1, np.int32))
    msg = impl.adam_step_ranges(b41, many, [0] * many, [4] * many, [LR] * many, [-1] * many, *tail)
    refused(msg, MSG["many"], "41 ranges")
    assert not b41["steps"].any()
    offs = list(c["offs"])
    offs[2] += 2
    refused(impl.adam_step_ranges(b, R, offs, c["lens"], lrs, c["gate_idx"], *tail), MSG["off"], "an offset of 2")
    nog = dict(b, gates=None)
    refused(impl.adam_step_ranges(nog, R, c["offs"], c["lens"], lrs, c["gate_idx"], *tail), MSG["gate"], "a gated range without gates")
    for name in ADAM_BUFFERS:
        refused(impl.adam_step_ranges(b, R, c["offs"], c["lens"], lrs, c["gate_idx"], *tail, misalign=name), MSG["align_r"], name + " misaligned")
    n = 12
    for name in ADAM_BUFFERS:
        msg = impl.adam_step(b, n, LR, B1, B2, EPS, 1.0 - B1, 1.0 - B2, 1.0, misalign=name)
        refused(msg, MSG["align"], "l4d_adam_step: " + name + " misaligned")


# =================================================================================================================================
# cast
# =================================================================================================================================
def cast_values():
    """fp32 inputs: every fp16 value widened, the midpoints between adjacent fp16 values (65520 = the one towards inf included)
    and their fp32 neighbours, both signs, the overflow threshold, the subnormal range and below half its smallest value."""
    h = np.arange(65536, dtype=np.uint16).view(F16).astype(F32)
    pos = np.arange(0x7c00 + 1, dtype=np.uint16).view(F16).astype(F64)     # 0 .. 65504, inf
    pos[-1] = 65536.0
    mid = ((pos[:-1] + pos[1:]) / 2).astype(F32)
    assert (mid.astype(F64) == (pos[:-1] + pos[1:]) / 2).all()
    around = np.concatenate([mid, np.nextafter(mid, F32(np.inf)), np.nextafter(mid, F32(0.0))])
    tiny = np.array([2.0 ** -25, 2.0 ** -26, 1e-30, 2.0 ** -149, 2.0 ** -24, 1.5 * 2.0 ** -25, 2.5 * 2.0 ** -25], F64).astype(F32)
    tiny = np.concatenate([tiny, np.nextafter(tiny[:1], F32(1.0)), np.nextafter(tiny[:1], F32(0.0))])
    special = np.array([65504.0, 65519.996, 65520.0, -65520.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e38, -3.4028235e38], F32)
    return np.concatenate([special, tiny, -tiny, around, -around, h])


CAST_SIZES = tuple(range(1, 10)) + (1023, 1024, 1025)


def check_cast(impl):
    x = cast_values()
    with np.errstate(all="ignore"):
        want = x.astype(F16)
    assert want[2] == np.inf and want[0] == 65504 and want[1] == 65504 and np.isnan(want[8]) and np.signbit(want[5])
    dst = np.full(x.size + GUARD, SENT_H, F16)
    assert impl.cast(x.copy(), dst, x.size) is None
    bad = np.flatnonzero(~same_bits(dst[:x.size], want))
    assert bad.size == 0, f"cast: {bad.size} of {x.size} differ, first inputs {x[bad[:6]]}: got {dst[bad[:6]]}, want {want[bad[:6]]}"
    assert same_bits(dst[x.size:], np.full(GUARD, SENT_H, F16)).all()
    for n in CAST_SIZES + (0,):
        src = x[7:7 + n + GUARD].copy()      # the special values, then midpoints
        dst = np.full(n + GUARD, SENT_H, F16)
        assert impl.cast(src, dst, n) is None
        assert same_bits(dst[:n], want[7:7 + n]).all(), f"cast n={n}"
        assert same_bits(dst[n:], np.full(GUARD, SENT_H, F16)).all(), f"cast n={n}: the guard behind dst was written"
        assert same_bits(src, x[7:7 + n + GUARD]).all()
    for which in ("src", "dst"):
        dst = np.full(16 + GUARD, SENT_H, F16)
        msg = impl.cast(x[:16 + GUARD].copy(), dst, 16, misalign=which)
        assert msg is not None and MSG["cast"] in msg, msg
        assert same_bits(dst, np.full(16 + GUARD, SENT_H, F16)).all()


# =================================================================================================================================
# non-finite check and absmax
# =================================================================================================================================
REDUCE_SMALL = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025)
NONFINITE_CAP, ABSMAX_CAP = 2048, 256            # workgroups of 256 lanes x 4 elements per sweep
NONFINITE_BIG = NONFINITE_CAP * 1024 * 2 + 3
ABSMAX_BIG = ABSMAX_CAP * 1024 * 2 + 3


def clean_input(n):
    """Finite values in +-100, with -0.0 and subnormals at the front (absmax needs a known largest value: no extremes here)."""
    x = (rng_of(43, n).uniform(-100.0, 100.0, size=n)).astype(F32)
    plant = np.array([-0.0, 2.0 ** -149, -(2.0 ** -130), 0.0], F32)
    k = min(n, plant.size)
    x[:k] = plant[:k]
    return x


def clean_extremes(n):
    """clean_input with +-3.4028235e38 planted too (cycled through for the small sizes): finite, so the flag stays down."""
    x = clean_input(n)
    plant = np.array([3.4028235e38, -3.4028235e38], F32)
    for j in range(min(n, 2)):
        x[(n // 2 + j) % n] = plant[j]
    if n >= 8:
        x[-1], x[-2] = plant[1], plant[0]
    return x


def positions(n, cap):
    """Index 0, the last, every position of the scalar tail, both sides of the lane 63 / lane 0 boundary of a wave, the last
    element of the first sweep and the first of the second."""
    sweep = cap * 1024
    p = {0, n - 1, 255, 256, sweep - 1, sweep} | set(range(n - n % 4, n)) | {n - n % 4 - 1}
    return sorted(i for i in p if 0 <= i < n)


def check_nonfinite(impl, n):
    state0 = np.array([3.0, 5.0, 0.0, 0.25], F32)
    x = clean_extremes(n)
    for base in (x, clean_input(n)):
        state = state0.copy()
        assert impl.nonfinite(base, [], n, state) is None
        assert same_bits(state, state0).all(), f"n={n}: clean input, state {state}"
    want = state0.copy()
    want[2] = 1.0
    for i in positions(n, NONFINITE_CAP):
        for v in (np.inf, -np.inf, np.nan):
            state = state0.copy()
            assert impl.nonfinite(x, [(i, F32(v))], n, state) is None
            assert same_bits(state, want).all(), f"n={n}: {v} at {i}: state {state}"


def check_absmax(impl, n):
    x = clean_input(n)
    out = np.array([SENT_P, SENT_M], F32)
    assert impl.absmax(x, [], n, out) is None
    assert same_bits(out, np.array([np.abs(x).max(), SENT_M], F32)).all(), f"n={n}: clean input, out {out}"
    for i in positions(n, ABSMAX_CAP):
        for v, want in ((np.inf, np.inf), (-np.inf, np.inf), (np.nan, np.inf), (-1000.5, 1000.5), (-3.4028235e38, 3.4028235e38)):
            out = np.array([SENT_P, SENT_M], F32)
            assert impl.absmax(x, [(i, F32(v))], n, out) is None
            assert same_bits(out, np.array([want, SENT_M], F32)).all(), f"n={n}: {v} at {i}: out {out}"


def check_reduce_edges(impl):
    """n = 0, all zeros, one subnormal, misaligned input."""
    state0 = np.array([3.0, 5.0, 0.0, 0.25], F32)
    state = state0.copy()
    assert impl.nonfinite(np.full(4, np.nan, F32), [], 0, state) is None and same_bits(state, state0).all()
    msg = impl.nonfinite(np.full(16, np.nan, F32), [], 12, state, misalign=True)
    assert msg is not None and MSG["nonfinite"] in msg and same_bits(state, state0).all()
    for x, want in ((np.zeros(1025, F32), 0.0), (np.full(1025, -0.0, F32), 0.0), (np.array([0, 0, -(2.0 ** -149), 0, 0], F32), 2.0 ** -149),
                    (np.array([2.0 ** -140], F32), 2.0 ** -140)):
        out = np.array([SENT_P, SENT_M], F32)
        assert impl.absmax(x, [], x.size, out) is None
        assert same_bits(out, np.array([want, SENT_M], F32)).all(), (x[:5], out)
    out = np.array([SENT_P, SENT_M], F32)
    assert impl.absmax(np.full(4, np.nan, F32), [], 0, out) is None and same_bits(out, np.array([0.0, SENT_M], F32)).all()
    msg = impl.absmax(np.full(16, 1.0, F32), [], 12, out, misalign=True)
    assert msg is not None and MSG["absmax"] in msg and same_bits(out[1:], np.array([SENT_M], F32)).all()


# =================================================================================================================================
# scaler update and slice gates
# =================================================================================================================================
def scaler_rule64(scale, tracker, found, growth, backoff, interval):
    """torch.amp.GradScaler.update() as documented, in float64: a step with a non-finite gradient multiplies the scale by
    backoff_factor and clears the tracker; growth_interval consecutive clean steps multiply it by growth_factor."""
    if found:
        return scale * backoff, 0
    tracker += 1
    if tracker == interval:
        return scale * growth, 0
    return scale, tracker


SCALER_RUNS = [  # (initial scale, growth, backoff, interval, found flags)
    (65536.0, 2.0, 0.5, 3, [1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1]),
    (1024.0, 2.0, 0.5, 1, [0, 0, 1, 0, 0]),
    (3.0, 1.5, 0.25, 2, [0, 0, 1, 0, 0, 0, 0]),
    (2.0 ** -125, 2.0, 0.5, 2000, [1, 1, 1, 1, 0]),          # through 2^-126 into the subnormals: 1 / scale = 2^127, then inf
    (2.0 ** 126, 2.0, 0.5, 1, [0, 0, 0, 1]),                  # past 2^127 to inf, 1 / scale = 0; inf * 0.5 stays inf
]


def check_scaler(impl):
    for scale0, growth, backoff, interval, founds in SCALER_RUNS:
        state = np.array([scale0, 0.0, 0.0, 1.0 / scale0], F32)
        scale, tracker = float(scale0), 0
        for k, found in enumerate(founds):
            state[2] = found * 7.0      # any non-zero value is "found"
            assert impl.scaler_update(state, growth, backoff, interval) is None
            scale, tracker = scaler_rule64(scale, tracker, found, growth, backoff, interval)
            with np.errstate(all="ignore"):
                scale = float(F32(scale))    # the state is fp32
                want = np.array([scale, tracker, 0.0, np.float64(1.0) / np.float64(scale) if scale else np.inf], F64).astype(F32)
            assert same_bits(state, want).all(), f"scaler from {scale0}, update {k} (found={found}): {state} != {want}"
    return True


SLICE_COUNTS = (1, 2, 5, 8)
GATE_PAD = 8


def slice_times(n_slices):
    ts = {F32(0.0), F32(1.0)} | {F32(k / (n_slices - 1)) for k in range(n_slices)} if n_slices > 1 else {F32(0.0), F32(1.0), F32(0.5)}
    out = set()
    for t in ts:
        out |= {t, np.nextafter(t, F32(2.0)), np.nextafter(t, F32(-1.0))}
    return sorted(out)


def check_slices(impl):
    """Exactly the gates of hashgrid_cases.slice_pair_f32 become 1.0; every other float of the buffer keeps its sentinel."""
    from hashgrid_cases import slice_pair_f32
    for n in SLICE_COUNTS:
        for t in slice_times(n):
            i1, i2, _, _ = slice_pair_f32(t, n)
            assert -1 <= i1 <= i2 <= n, (t, n, i1, i2)     # inside the padding
            gates = np.full(n + 2 * GATE_PAD, SENT_G, F32)
            assert impl.mark_time_slices(F32(t), n, gates, GATE_PAD) is None
            want = np.full(n + 2 * GATE_PAD, SENT_G, F32)
            want[GATE_PAD + i1] = want[GATE_PAD + i2] = 1.0
            assert same_bits(gates, want).all(), f"n_slices={n} t={float(t)!r}: gates {gates[GATE_PAD - 1:GATE_PAD + n + 1]}, expected slices {i1}, {i2}"
