"""Edge tests of the optimiser kernels on the device (``-m gpu``, MI355X): l4d_adam_step, l4d_adam_step_ranges,
l4d_cast_f32_to_f16, l4d_grad_nonfinite_check, l4d_absmax_f32, l4d_scaler_update and l4d_mark_time_slices through the C ABI, with
buffers the tests allocate and prefill, so that what a kernel must not write is seen.

The check bodies, the cases, the float64 reference of Adam and the derivation of its bounds are in tests/optim_cases.py;
tests/test_optim_cpu.py runs the same bodies against a float32 restatement of the kernels, with and without faults."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ADAM_KEYS = ("param", "grad", "exp_avg", "exp_avg_sq", "param_f16", "gates", "scaler", "steps", "sched")


def _up(a, misalign=False):
    """numpy -> device; misalign: one element behind the start of a fresh allocation."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.to(DEV)
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=DEV)
    view = buf[1:1 + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


class Device:
    """optim_cases' implementation interface over ops.call: upload, one call, synchronise, download into the same arrays."""

    def __init__(self):
        self._base = (None, None)

    @staticmethod
    def _call(name, *args):
        from lidar4d_amd import ops
        from lidar4d_amd._lib import HipExtensionError
        try:
            ops.call(name, *args, ops._stream())
        except HipExtensionError as e:
            torch.cuda.synchronize()
            return str(e)
        torch.cuda.synchronize()
        return None

    @staticmethod
    def _down(b, d):
        for k, t in d.items():
            if t is not None:
                b[k][...] = t.cpu().numpy()

    def adam_step(self, b, n, lr, b1, b2, eps, bias_c1, bias_c2, grad_scale, misalign=None):
        from lidar4d_amd.ops import _p
        d = {k: _up(b[k], misalign == k) for k in oc.ADAM_BUFFERS}
        msg = self._call("l4d_adam_step", _p(d["param"]), _p(d["grad"]), _p(d["exp_avg"]), _p(d["exp_avg_sq"]), _p(d["param_f16"]), n,
                         lr, b1, b2, eps, bias_c1, bias_c2, grad_scale)
        self._down(b, d)
        return msg

    def adam_step_ranges(self, b, n_ranges, off, ln, lr, gate_idx, b1, b2, eps, grad_scale, sched_iters, misalign=None):
        from lidar4d_amd.ops import _i32s, _i64s, _p
        d = {k: _up(b[k], misalign == k) for k in ADAM_KEYS}
        lrs = (C.c_float * len(lr))(*lr)
        msg = self._call("l4d_adam_step_ranges", _p(d["param"]), _p(d["grad"]), _p(d["exp_avg"]), _p(d["exp_avg_sq"]), _p(d["param_f16"]),
                         n_ranges, _i64s(list(off)), _i64s(list(ln)), C.cast(lrs, C.c_void_p), None if gate_idx is None else _i32s(list(gate_idx)),
                         _p(d["gates"]), _p(d["scaler"]), _p(d["steps"]), b1, b2, eps, grad_scale, _p(d["sched"]), float(sched_iters))
        self._down(b, d)
        return msg

    def cast(self, src, dst, n, misalign=None):
        from lidar4d_amd.ops import _p
        d = dict(src=_up(src, misalign == "src"), dst=_up(dst, misalign == "dst"))
        msg = self._call("l4d_cast_f32_to_f16", _p(d["src"]), _p(d["dst"]), n)
        self._down(dict(src=src, dst=dst), d)
        return msg

    def _input(self, x, pokes, misalign):
        if misalign:
            return _up(x, True)
        if self._base[0] is not x:            # the large inputs are uploaded once and poked on the device
            self._base = (x, _up(x))
        t = self._base[1]
        if pokes:
            t = t.clone()
            for i, v in pokes:
                t[i] = float(v)
        return t

    def nonfinite(self, x, pokes, n, state, misalign=False):
        from lidar4d_amd.ops import _p
        t, s = self._input(x, pokes, misalign), _up(state)
        msg = self._call("l4d_grad_nonfinite_check", _p(t), n, _p(s))
        state[...] = s.cpu().numpy()
        return msg

    def absmax(self, x, pokes, n, out, misalign=False):
        from lidar4d_amd.ops import _p
        t, o = self._input(x, pokes, misalign), _up(out)
        msg = self._call("l4d_absmax_f32", _p(t), n, _p(o))
        out[...] = o.cpu().numpy()
        return msg

    def scaler_update(self, state, growth, backoff, interval):
        from lidar4d_amd.ops import _p
        s = _up(state)
        msg = self._call("l4d_scaler_update", _p(s), growth, backoff, interval)
        state[...] = s.cpu().numpy()
        return msg

    def mark_time_slices(self, t, n_slices, gates, base):
        from lidar4d_amd.ops import _p
        tinfo, g = _up(np.array([t, 0.0, 0.0, 0.0], F32)), _up(gates)
        msg = self._call("l4d_mark_time_slices", _p(tinfo), n_slices, _p(g[base:]))   # slice 0 at gates[base]: padding on both sides
        gates[...] = g.cpu().numpy()
        return msg


@pytest.fixture(scope="module")
def impl():
    return Device()


# ---- Adam -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.RANGES_CASES)
def test_adam_ranges_against_float64(impl, name):
    spare = oc.check_adam_ranges(impl, name)
    print(f"{name}: smallest bound / error: parameter {spare[0]:.1f}, exp_avg {spare[1]:.1f}, exp_avg_sq {spare[2]:.1f}")


@pytest.mark.parametrize("n", oc.ADAM_LENGTHS)
def test_adam_flat_against_float64(impl, n):
    spare = oc.check_adam_flat(impl, n)
    print(f"n={n}: smallest bound / error: parameter {spare[0]:.1f}, exp_avg {spare[1]:.1f}, exp_avg_sq {spare[2]:.1f}")
    if n in (3, 1025):
        oc.check_adam_flat(impl, n, with_f16=False)


def test_adam_gradient_values(impl):
    oc.check_adam_values(impl)


def test_adam_noops_and_the_skip_flag(impl):
    oc.check_adam_noops_and_skip(impl)


def test_adam_refusals_write_nothing(impl):
    oc.check_adam_refusals(impl)


# ---- cast, reductions, scaler, gates ----------------------------------------------------------------------------------------------
def test_cast_is_round_to_nearest_even(impl):
    oc.check_cast(impl)


@pytest.mark.parametrize("n", oc.REDUCE_SMALL + (oc.NONFINITE_BIG,))
def test_nonfinite_check_positions(impl, n):
    oc.check_nonfinite(impl, n)


@pytest.mark.parametrize("n", oc.REDUCE_SMALL + (oc.ABSMAX_BIG,))
def test_absmax_positions(impl, n):
    oc.check_absmax(impl, n)


def test_reductions_edges(impl):
    oc.check_reduce_edges(impl)


def test_scaler_update_follows_the_gradscaler_rule(impl):
    oc.check_scaler(impl)


def test_mark_time_slices(impl):
    oc.check_slices(impl)
