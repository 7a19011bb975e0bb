"""The width-generic fused MLP (csrc/mlp_width.hip, liblidar4d_mlp.so: hidden widths 16, 32 and 128) on the GPU.

Kernel level: every comparison is torch.equal against the float64 reference on the integer lattice of tests/mlp_width_ref.py
(every product, every sum in any order and every rounding exact: asserted on the CPU, tests/test_mlp_width_cpu.py) -- all 72
(hidden, in_pad, n_hidden) shapes, ragged and device row counts, the grid-stride loops, the caller's state (grad_w accumulation,
dx == null, sentinels past the end), dx_absmax, the ReLU gate at +-0.  Above it: ``tcnn.Network`` at each width, ``LiDAR4D`` with
mixed widths (render, gradients, operator-level modules) and a ``Trainer`` against the oracle and against the eager step, and a
default-width model that never maps the new library.  Run with ``-m gpu`` on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_width_ref as mw
from oracle import fields_ref, tcnn_ref
from oracle.detparams import det_uniform, fill_model, grad_digest
from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENT = 0x5A5A  # bit pattern of rows the kernels must leave alone (as fp16: 203.25, a value that would open a ReLU gate)
EDGE_SHAPES = [(16, 16, 2), (32, 96, 2), (128, 192, 3), (128, 128, 1)]
# Rows per pass of the grid-stride loops (csrc/mlp_width.hip, "Workgroups per launch"): forward 1024 workgroups x 4 wavefronts x 16
# rows = 65,536 at widths 16 / 32 and 256 x 4 x 16 = 16,384 at width 128; backward 512 x 4 x 32 = 65,536 at widths 16 / 32, and at
# width 128 256 x 32 = 8,192 (weight gradients) and 256 x 4 x 32 = 32,768 (dx).  65,573 rows exceed every one of them, with a ragged
# last tile; the lattice is exact there (tests/test_mlp_width_cpu.py::test_lattice_is_exact_at_the_grid_stride_row_count).
LARGE_P = 65573
HALF_ULP = 2.0 ** -10
MIXED = [dict(hidden_dim_sigma=32, hidden_dim_lidar=128, hidden_dim_flow=16),
         dict(hidden_dim_sigma=128, hidden_dim_lidar=16, hidden_dim_flow=32)]


def ops_():
    from lidar4d_amd import ops
    return ops


def sent16(*shape):
    return torch.full(shape, SENT, dtype=torch.int16, device=DEV).view(torch.float16)


def untouched(t):
    return bool((t.view(torch.int16) == SENT).all())


def eq16(got, ref):
    got = got.cpu()
    return got.dtype == torch.float16 and torch.equal(got, mw.t16(ref))


def eq32(got, ref):
    got = got.cpu()
    return got.dtype == torch.float32 and torch.equal(got, mw.t32(ref))


def with_nan_past(a, n):
    """fp16 device copy of the lattice array whose rows from n on are NaN: rows the kernels may not look at."""
    t = mw.t16(a).clone()
    t[n:] = float("nan")
    return t.to(DEV)


def sigma_ok(sigma, y_ref):
    """sigma = exp(fp16 y0) at fp32 expf accuracy (4 ulp); beyond the fp32 range: inf, or (nearly) zero."""
    want = np.exp(np.clip(y_ref[:, 0], -200.0, 200.0))
    got = sigma.double().cpu().numpy()
    mid = (want > 1e-30) & (want < 1e38)
    return (bool((np.abs(got[mid] - want[mid]) <= 2.0 ** -21 * want[mid]).all()) and bool(np.isinf(got[want >= 3.5e38]).all())
            and bool((got[want <= 1e-30] <= 1e-30).all()))


def fwd_bwd_equal(c, x, w, dy, inv=1.0):
    """One forward and one backward on the whole case; everything equal to the reference."""
    ops = ops_()
    y, act = ops.mlp_fwd(x, w, c.n_hidden, save_act=True, hidden=c.hidden)
    assert act.shape == (c.n_hidden, c.P, c.hidden)
    assert eq16(y, c.y), "y"
    assert eq16(act, c.act), "act"
    g = torch.zeros(w.numel(), device=DEV)
    dx = ops.mlp_bwd(x, act, dy, w, c.n_hidden, g, inv, hidden=c.hidden)
    assert eq16(dx, c.dx), "dx"
    assert eq32(g, c.grad(None, inv)), "grad_w"
    return act


# ---- a. all 72 shapes, ragged rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [131, 33])
@pytest.mark.parametrize("hidden,in_pad,n_hidden", mw.SHAPES)
def test_every_shape_equals_float64(hidden, in_pad, n_hidden, P):
    ops = ops_()
    c = mw.case(hidden, in_pad, n_hidden, P)
    c.stats_ok()
    x, w, dy = mw.t16(c.x).to(DEV), c.w16().to(DEV), mw.t16(c.dy).to(DEV)
    fwd_bwd_equal(c, x, w, dy)
    y, act, sigma = ops.mlp_fwd_sigma(x, w, n_hidden, save_act=True, hidden=hidden)
    assert eq16(y, c.y) and eq16(act, c.act)
    assert sigma.shape == (P,) and sigma.dtype == torch.float32 and sigma_ok(sigma, c.y)
    y2, none = ops.mlp_fwd(x, w, n_hidden, save_act=False, hidden=hidden)
    assert none is None and eq16(y2, c.y), "y (no activations stored)"


def test_unsupported_shapes_are_refused():
    from lidar4d_amd import _mlp_lib
    from lidar4d_amd._lib import HipExtensionError
    ops = ops_()
    x = torch.zeros(8, 48, dtype=torch.float16, device=DEV)
    w = torch.zeros(32 * 48 + 16 * 32, dtype=torch.float16, device=DEV)
    with pytest.raises(HipExtensionError, match="unsupported shape"):
        ops.mlp_fwd(x, w, 1, hidden=32)
    x = torch.zeros(8, 32, dtype=torch.float16, device=DEV)
    with pytest.raises(HipExtensionError, match="unsupported shape"):
        ops.mlp_fwd(x, w, 4, hidden=32)
    y = torch.zeros(8, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(HipExtensionError, match="unsupported shape"):  # width 64 is the other library's
        _mlp_lib.call("l4dm_mlp_fwd", ops._p(x), 8, None, 32, 64, 1, ops._p(w), ops._p(y), None, None, ops._stream())
    with pytest.raises(ValueError, match="stored activations"):
        ops.mlp_bwd(x, None, y, w, 1, torch.zeros(w.numel(), device=DEV), 1.0, hidden=32)


# ---- b. row-count edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 15, 16, 17, 31, 32, 33, 63, 65])
@pytest.mark.parametrize("hidden,in_pad,n_hidden", EDGE_SHAPES)
def test_row_count_edges(hidden, in_pad, n_hidden, P):
    ops = ops_()
    c = mw.case(hidden, in_pad, n_hidden, P)
    w = c.w16().to(DEV)
    fwd_bwd_equal(c, mw.t16(c.x).to(DEV), w, mw.t16(c.dy).to(DEV))
    for n in sorted({0, 1, P - 1, P, P + 100}):
        m = min(n, P)
        n_rows = torch.tensor([n], dtype=torch.int32, device=DEV)
        x, dy = with_nan_past(c.x, m), with_nan_past(c.dy, m)
        y, act, dx = sent16(P, 16), sent16(n_hidden, P, hidden), sent16(P, in_pad)
        sigma = torch.full((P,), -7.0, device=DEV)
        ops.mlp_fwd(x, w, n_hidden, save_act=True, n_rows=n_rows, y=y, act=act, hidden=hidden, sigma=sigma)
        assert eq16(y[:m], c.y[:m]) and eq16(act[:, :m], c.act[:, :m]), (n, "forward")
        assert untouched(y[m:]) and untouched(act[:, m:]) and bool((sigma[m:] == -7.0).all()), (n, "forward wrote past the row count")
        assert sigma_ok(sigma[:m], c.y[:m])
        act_nan = act.clone()
        act_nan[:, m:] = float("nan")
        g = torch.full((w.numel(),), 3.0, device=DEV)
        ops.mlp_bwd(x, act_nan, dy, w, n_hidden, g, 1.0, n_rows=n_rows, dx=dx, hidden=hidden)
        assert eq16(dx[:m], c.dx[:m]), (n, "dx")
        assert untouched(dx[m:]), (n, "backward wrote past the row count")
        assert eq32(g, c.grad(m) + 3.0), (n, "grad_w")  # n = 0: unchanged


# ---- c. grid-stride loops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", mw.WIDTHS)
def test_grid_stride(hidden):
    """65,573 rows: more than one pass of every launch's grid-stride loop (LARGE_P above), so wavefronts take several tiles and
    the last tile is ragged."""
    c = mw.case(hidden, 96, 2, LARGE_P)
    c.stats_ok()
    fwd_bwd_equal(c, mw.t16(c.x).to(DEV), c.w16().to(DEV), mw.t16(c.dy).to(DEV), inv=1.0 / 128)


# ---- d. the caller's state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,in_pad,n_hidden", EDGE_SHAPES)
def test_grad_w_accumulates_into_callers_state(hidden, in_pad, n_hidden):
    ops = ops_()
    c = mw.case(hidden, in_pad, n_hidden, 131)
    x, w, dy = mw.t16(c.x).to(DEV), c.w16().to(DEV), mw.t16(c.dy).to(DEV)
    _, act = ops.mlp_fwd(x, w, n_hidden, save_act=True, hidden=hidden)
    prefill = mw.lattice_ints((w.numel(),), 3, (hidden, in_pad, n_hidden, 7))
    for inv in (1.0, 1.0 / 128):
        g = mw.t32(prefill).to(DEV)
        dx = ops.mlp_bwd(x, act, dy, w, n_hidden, g, inv, hidden=hidden)
        assert eq16(dx, c.dx) and eq32(g, prefill + c.grad(None, inv)), inv
        g2 = mw.t32(prefill).to(DEV)
        assert ops.mlp_bwd(x, act, dy, w, n_hidden, g2, inv, want_dx=False, hidden=hidden) is None
        assert torch.equal(g2, g), (inv, "dx == null changes grad_w")
        g3 = torch.zeros(w.numel(), device=DEV)
        ops.mlp_bwd(x, act, dy, w, n_hidden, g3, inv, hidden=hidden)
        ops.mlp_bwd(x, act, dy, w, n_hidden, g3, inv, want_dx=False, hidden=hidden)
        assert eq32(g3, 2.0 * c.grad(None, inv)), (inv, "two calls into one grad_w")


# ---- e. dx_absmax -----------------------------------------------------------------------------------------------------------
ABSMAX_TILE_SCALE = {1: 4.0, 3: 16.0, 5: 8.0, 7: 4.0, 9: 4.0}  # W1's odd 16-column tiles; the even ones keep +-1


@pytest.mark.parametrize("hidden,in_pad,n_hidden,ranges", [(32, 128, 1, [(0, 16), (64, 128), (0, 128)]),
                                                           (128, 176, 2, [(0, 16), (64, 128), (0, 176), (96, 176)]),
                                                           (16, 64, 2, [(32, 48), (16, 64)])])
def test_dx_absmax(hidden, in_pad, n_hidden, ranges):
    """The lattice with the odd 16-column tiles of W1 scaled by powers of two, as tests/test_gpu_mlp_exact.py has it: a column
    range that is one tile too wide at either end gives a wrong number."""
    from lidar4d_amd._lib import HipExtensionError
    ops = ops_()
    P, n = 131, 77
    Ws = mw.lattice_weights(hidden, in_pad, n_hidden)
    for tile, f in ABSMAX_TILE_SCALE.items():
        Ws[0][:, 16 * tile:16 * tile + 16] *= f
    c = mw.Case(hidden, in_pad, n_hidden, P, Ws=Ws)
    wants = [float(np.abs(c.dx[:, lo:hi]).max()) for lo, hi in ranges]
    assert len(set(wants)) == len(wants), ("every range has a maximum of its own", wants)
    tile_max = [float(np.abs(c.dx[:, 16 * t:16 * t + 16]).max()) for t in range(in_pad // 16)]
    for t in range(0, in_pad // 16, 2):  # an even tile alone: one tile too many at either end raises the maximum
        assert all(tile_max[u] > tile_max[t] > 0 for u in (t - 1, t + 1) if 0 <= u < in_pad // 16), tile_max
    ranges = ranges + [(16 * t, 16 * t + 16) for t in range(in_pad // 16) if (16 * t, 16 * t + 16) not in ranges]
    x, w, dy = mw.t16(c.x).to(DEV), c.w16().to(DEV), mw.t16(c.dy).to(DEV)
    _, act = ops.mlp_fwd(x, w, n_hidden, save_act=True, hidden=hidden)
    g = torch.zeros(w.numel(), device=DEV)
    n_rows = torch.tensor([n], dtype=torch.int32, device=DEV)
    x_n, dy_n = with_nan_past(c.x, n), with_nan_past(c.dy, n)
    live = int(np.argmax((c.act > 0).sum(2).min(0)))  # a row with active units in every layer: an inf in its dy reaches dx
    assert (c.act[:, live] > 0).any(1).all()
    dy_inf = dy.clone()
    dy_inf[live, 3] = float("inf")
    for lo, hi in ranges:
        want = float(np.abs(c.dx[:, lo:hi]).max())
        assert want > 0
        amax = torch.zeros(1, device=DEV)
        dx = ops.mlp_bwd(x, act, dy, w, n_hidden, g, 1.0, dx_absmax=amax, absmax_cols=(lo, hi), hidden=hidden)
        assert eq16(dx, c.dx) and float(amax) == want, (lo, hi, float(amax), want)
        big = torch.full((1,), want + 0.5, device=DEV)  # a larger value already there is kept
        ops.mlp_bwd(x, act, dy, w, n_hidden, g, 1.0, dx_absmax=big, absmax_cols=(lo, hi), hidden=hidden)
        assert float(big) == want + 0.5
        small = torch.full((1,), 0.25, device=DEV)  # a smaller one is raised
        ops.mlp_bwd(x, act, dy, w, n_hidden, g, 1.0, dx_absmax=small, absmax_cols=(lo, hi), hidden=hidden)
        assert float(small) == want
        want_n = float(np.abs(c.dx[:n, lo:hi]).max())  # rows past the device row count do not count
        amax = torch.zeros(1, device=DEV)
        ops.mlp_bwd(x_n, act, dy_n, w, n_hidden, g, 1.0, n_rows=n_rows, dx_absmax=amax, absmax_cols=(lo, hi), hidden=hidden)
        assert float(amax) == want_n, (lo, hi, float(amax), want_n)
        amax = torch.zeros(1, device=DEV)
        ops.mlp_bwd(x, act, dy_inf, w, n_hidden, torch.zeros_like(g), 1.0, dx_absmax=amax, absmax_cols=(lo, hi), hidden=hidden)
        assert float(amax) == float("inf"), (lo, hi, float(amax))
    amax = torch.zeros(1, device=DEV)
    for bad in ((8, 32), (0, 24), (0, in_pad + 16), (-16, 16)):
        with pytest.raises(HipExtensionError, match="dx_absmax needs dx and a column range"):
            ops.mlp_bwd(x, act, dy, w, n_hidden, g, 1.0, dx_absmax=amax, absmax_cols=bad, hidden=hidden)
    with pytest.raises(HipExtensionError, match="dx_absmax needs dx and a column range"):
        ops.mlp_bwd(x, act, dy, w, n_hidden, g, 1.0, want_dx=False, dx_absmax=amax, absmax_cols=ranges[0], hidden=hidden)
    assert float(amax) == 0.0


# ---- f. the ReLU gate at +-0 ------------------------------------------------------------------------------------------------
TINY = 2.0 ** -13  # a normal fp16 number whose square, 2^-26, is below half the smallest fp16 subnormal: it rounds to (+-)0
KINDS = ("neg_tiny", "pos_tiny", "zero", "pos", "neg")  # pre-activation -2^-26, +2^-26, exactly 0, +3, -3
GATE_ROWS = (0, 13, 37, 69)  # the rows that carry anything: both halves of a 32-row macro tile, three tiles, the ragged last row
CARRIER = 5  # (n_hidden = 2) the layer-1 unit whose activation is 2^-13: the tiny products of layer 2 come from it


def kind_of(m):
    return KINDS[m % 5]  # neighbours differ: the packed fp16 pairs mix a -0 with every other kind


def gate_problem(H, n_hidden):
    """tests/test_gpu_mlp_exact.py::gate_problem at hidden width H: x [70, 16] (zero but for GATE_ROWS: column 0 = 2^-13, columns
    1, 2 = 3), weights that put every hidden unit of the gated layer(s) into one of KINDS, dy = 1 and an output layer that hands
    every unit of the last hidden layer dh = 1."""
    P = 70
    x = np.zeros((P, 16))
    x[list(GATE_ROWS), 0], x[list(GATE_ROWS), 1], x[list(GATE_ROWS), 2] = TINY, 3.0, 3.0
    W1 = np.zeros((H, 16))
    kinds1 = []
    for m in range(H):
        k = "carrier" if (n_hidden == 2 and m == CARRIER) else kind_of(m)
        kinds1.append(k)
        if k == "carrier":
            W1[m, 0] = 1.0
        elif k == "neg_tiny":
            W1[m, 0] = -TINY
        elif k == "pos_tiny":
            W1[m, 0] = TINY
        elif k == "zero":
            W1[m, 1], W1[m, 2] = 1.0, -1.0
        elif k == "pos":
            W1[m, 1 + (m & 1)] = 1.0
        else:
            W1[m, 1 + (m & 1)] = -1.0
    Ws, kinds = [W1], [kinds1]
    if n_hidden == 2:
        pos1 = [m for m in range(H) if kinds1[m] == "pos"]
        dead1 = [m for m in range(H) if kinds1[m] in ("neg_tiny", "pos_tiny", "zero", "neg")]
        assert len(pos1) >= 2
        W2 = np.zeros((H, H))
        for m in range(H):
            k = kind_of(m)
            if k == "neg_tiny":
                W2[m, CARRIER] = -TINY
            elif k == "pos_tiny":
                W2[m, CARRIER] = TINY
            elif k == "zero":
                W2[m, pos1[0]], W2[m, pos1[1]] = 1.0, -1.0
            elif k == "pos":  # (layer-1 unit m is live as well: at every width each live layer-1 unit feeds a live layer-2 unit)
                assert m in pos1
                W2[m, m] = 1.0
                W2[m, dead1] = 1.0  # a dead layer-1 unit adds nothing forward, and receives dh1 > 0: a leak would show
            else:
                W2[m, pos1[m % len(pos1)]] = -1.0
        Ws.append(W2)
        kinds.append([kind_of(m) for m in range(H)])
    Wo = np.zeros((16, H))
    Wo[np.arange(H) % 16, np.arange(H)] = 1.0
    Ws.append(Wo)
    return x, np.ones((P, 16)), Ws, kinds


@pytest.mark.parametrize("n_hidden", [1, 2])
@pytest.mark.parametrize("hidden", mw.WIDTHS)
def test_relu_gate_at_signed_zero(hidden, n_hidden):
    """A pre-activation of -2^-26 rounds to fp16 -0.  The stored activation must be +0, and no gradient may pass a unit at
    +-2^-26 or at 0 -- nor a unit whose stored activation is -0 (the gate is act > 0, not a bit pattern)."""
    ops = ops_()
    x64, dy64, Ws, kinds = gate_problem(hidden, n_hidden)
    y_ref, act_ref = mw.forward(x64, Ws, strict=False)
    dx_ref, dW_ref = mw.backward(x64, act_ref, dy64, Ws, strict=False)
    P = x64.shape[0]
    special = np.zeros(P, dtype=bool)
    special[list(GATE_ROWS)] = True
    for l in range(n_hidden):  # the reference itself: a unit is active exactly on the special rows, and only if "pos"/"carrier"
        for m in range(hidden):
            on = kinds[l][m] in ("pos", "carrier")
            assert ((act_ref[l][:, m] > 0) == (special & on)).all()
    assert (dx_ref[~special] == 0).all() and (dx_ref[special] != 0).any()
    x, w, dy = mw.t16(x64).to(DEV), torch.from_numpy(mw.pack(Ws)).to(DEV), mw.t16(dy64).to(DEV)
    y, act = ops.mlp_fwd(x, w, n_hidden, save_act=True, hidden=hidden)
    bits = act.view(torch.int16).cpu()
    assert bool((bits >= 0).all()), f"{int((bits < 0).sum())} stored activations carry a sign bit (-0)"
    assert eq16(y, y_ref) and eq16(act, act_ref)
    act_neg0 = torch.where(act == 0, torch.full_like(act, -0.0), act)  # the same activations with every zero as -0
    assert bool((act_neg0.view(torch.int16)[act == 0] < 0).all())
    for a in (act, act_neg0):
        g = torch.zeros(w.numel(), device=DEV)
        dx = ops.mlp_bwd(x, a, dy, w, n_hidden, g, 1.0, hidden=hidden)
        assert eq16(dx, dx_ref), "dx"
        assert eq32(g, dW_ref), "grad_w"
        gn, off = g.cpu().numpy(), 0
        for l in range(n_hidden):  # dW_l[m, :] shows unit m's gate alone: gradient reaches it iff the stored activation is > 0
            cols = Ws[l].shape[1]
            dWl = gn[off:off + hidden * cols].reshape(hidden, cols)
            off += hidden * cols
            for m in range(hidden):
                if kinds[l][m] == "pos":  # (the carrier is active, but feeds only units at +-2^-26: nothing comes back to it)
                    assert dWl[m].any(), (l, m, kinds[l][m])
                else:
                    assert not dWl[m].any(), (l, m, kinds[l][m], "gradient through a dead unit")
        assert not dx.cpu()[torch.from_numpy(~special)].any()


# ---- g. tcnn.Network against the oracle -------------------------------------------------------------------------------------
def rel_close(got, ref, rtol, atol, what="", frac_ok=0.0):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = (got - ref).abs() > atol + rtol * ref.abs()
    nbad = int(bad.sum())
    assert nbad <= frac_ok * bad.numel(), (
        f"{what}: {nbad}/{bad.numel()} out of tolerance; max abs err {(got - ref).abs().max():.3e}, ref max {ref.abs().max():.3e}")


@pytest.fixture()
def tcnn_mode():
    prev = tcnn_ref.get_precision()
    tcnn_ref.set_precision("tcnn")
    yield
    tcnn_ref.set_precision(prev)


def _f64_eval(ref, x):
    """The oracle's network in float64 on the same fp16 weights, rounded to fp16 where the oracle rounds."""
    rh64 = lambda v: v.to(torch.float16).to(torch.float64)
    in_pad = ref.shapes[0][1]
    x = x.double()
    if in_pad > x.shape[1]:
        x = torch.cat([x, torch.ones(x.shape[0], in_pad - x.shape[1], dtype=x.dtype)], -1)
    h, ws = rh64(x), [w.detach().double() for w in ref.weights()]
    for w in ws[:-1]:
        h = rh64(torch.relu(h @ w.t()))
    return rh64(h @ ws[-1].t())[:, :ref.n_output_dims]


@pytest.mark.parametrize("n_in,n_out,n_hidden", [(120, 16, 1), (87, 1, 2), (16, 6, 2)])
@pytest.mark.parametrize("width", mw.WIDTHS)
def test_network_vs_oracle(tcnn_mode, width, n_in, n_out, n_hidden):
    """tests/test_gpu_ops.py::test_mlp_fwd_bwd at the other widths, with that test's bounds: forward rtol 4 half-ulp, atol 2e-3, at
    most 1e-3 of the elements outside; gradients rtol 2e-2, atol 2e-3 x max.

    The atol is not widened for the wider network.  Measured on the CPU (this test's weights and inputs, P = 5,000, all three
    shapes): the oracle's own largest deviation from a float64 evaluation of the same fp16 weights, rounded where the oracle
    rounds, is 1.953e-3 at width 64 and 1.953e-3 at width 128 (one fp16 ulp of an output in [2, 4): the fp32 accumulation flips a
    rounding; 1.5e-3 .. 8.4e-3 of the outputs differ at all), so the ratio is 1.  No element of that comparison is outside
    rtol 4 half-ulp + atol 2e-3 at either width -- asserted below on the oracle itself, before the GPU result is looked at."""
    from lidar4d_amd import tcnn
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": n_hidden}
    ref = tcnn_ref.Network(n_in, n_out, cfg)
    mod = tcnn.Network(n_in, n_out, cfg)
    with torch.no_grad():
        ref.params.copy_(det_uniform((ref.params.numel(),), f"mlp{n_in}w{width}", -0.3, 0.3))
        mod.params.copy_(ref.params)
    mod = mod.to(DEV)
    P = 5000  # not a multiple of 16/32: exercises the ragged tail
    x = det_uniform((P, n_in), "mx", -1, 1).requires_grad_(True)
    xg = x.detach().to(DEV).requires_grad_(True)
    y_ref = ref(x)
    rel_close(y_ref.float(), _f64_eval(ref, x.detach()), rtol=4 * HALF_ULP, atol=2e-3, what="oracle vs float64", frac_ok=1e-3)
    y = mod(xg)
    assert y.dtype == torch.float16 and y.shape == (P, n_out)
    rel_close(y.float(), y_ref.float(), rtol=4 * HALF_ULP, atol=2e-3, what="mlp fwd", frac_ok=1e-3)
    g = det_uniform((P, n_out), "mg", -1, 1)
    y_ref.float().backward(g)
    y.backward(g.to(DEV).half())
    gmax = ref.params.grad.abs().max().item()
    rel_close(mod.params.grad, ref.params.grad, rtol=2e-2, atol=2e-3 * gmax, what="mlp dW")
    rel_close(xg.grad, x.grad, rtol=2e-2, atol=2e-3 * x.grad.abs().max().item(), what="mlp dX")


# ---- h. LiDAR4D with mixed widths against the oracle ------------------------------------------------------------------------
def scale_err(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("widths", MIXED)
def test_mixed_width_model_vs_oracle(tcnn_mode, widths):
    """The small configuration and the bounds of tests/test_gpu_model.py::test_render_variants_vs_oracle (outputs 1e-3 of their
    scale, gradient digests 3e-2), and of ::test_density_attribute_flow_modules for the operator-level density / attribute / flow."""
    from lidar4d_amd import LiDAR4D
    cfg = dict(SMALL_MODEL, density_scale=30.0, **widths)
    ref = fill_model(fields_ref.LiDAR4D(**cfg), seed=5)
    hip = fill_model(LiDAR4D(**cfg), seed=5).to(DEV)
    ro, rd = make_rays(48, 3)
    noise = det_uniform((48, 128), "vn", 0.0, 1.0)
    t = torch.tensor([[0.5]], dtype=torch.float32)
    o_ref = ref.render(ro, rd, t, num_steps=128, perturb=True, noise=noise)
    o = hip.render(ro.to(DEV), rd.to(DEV), t.to(DEV), num_steps=128, perturb=True, noise=noise.to(DEV))
    assert torch.equal(o["z_vals"].cpu(), o_ref["z_vals"])
    for k in ("depth_lidar", "image_lidar"):
        assert scale_err(o[k], o_ref[k]) < 1e-3, (k, scale_err(o[k], o_ref[k]))
    gd_, gi_ = det_uniform((1, 48), "vgd", -1, 1), det_uniform((1, 48, 2), "vgi", -1, 1)
    ((o_ref["depth_lidar"] * gd_).sum() + (o_ref["image_lidar"] * gi_).sum()).backward()
    ((o["depth_lidar"] * gd_.to(DEV)).sum() + (o["image_lidar"] * gi_.to(DEV)).sum()).backward()
    dig_ref, dig = grad_digest(ref), grad_digest(hip)
    for n, v in dig_ref.items():
        scale = max(abs(v[1]), 1e-12)
        assert max(abs(dig[n][k] - v[k]) for k in range(3)) / scale < 3e-2, (n, dig[n], v)
    for net in ("sigma_net.params", "intensity_net.params", "raydrop_net.params", "flow_net.mlp.0.weight"):
        assert abs(dig_ref[net][1]) > 0, net
    # operator level
    pts = det_uniform((3000, 3), "dpts", -1.0, 1.0)
    ref.zero_grad()
    hip.zero_grad()
    d_ref = ref.density(pts, t)
    d = hip.density(pts.to(DEV), t.to(DEV))
    rel = ((d["sigma"].cpu() - d_ref["sigma"]).abs() / d_ref["sigma"].abs()).detach()
    assert float(rel.max()) < 2 ** -8 and float((rel > 1e-5).float().mean()) < 0.02, (float(rel.max()), float((rel > 1e-5).float().mean()))
    gerr = (d["geo_feat"].float().cpu() - d_ref["geo_feat"].float()).abs().detach()
    assert float(gerr.max()) <= 2 ** -8 and float((gerr > 0).float().mean()) < 0.02
    gsig, ggeo = det_uniform((3000,), "gs", -1, 1), det_uniform((3000, 15), "gg", -1, 1)
    ((d_ref["sigma"] * gsig).sum() + (d_ref["geo_feat"].float() * ggeo).sum()).backward()
    ((d["sigma"] * gsig.to(DEV)).sum() + (d["geo_feat"].float() * ggeo.to(DEV)).sum()).backward()
    dig_ref, dig = grad_digest(ref), grad_digest(hip)
    for n, v in dig_ref.items():
        scale = max(abs(v[1]), 1e-12)
        assert max(abs(dig[n][k] - v[k]) for k in range(3)) / scale < 3e-2, (n, dig[n], v)
    f_ref, f = ref.flow(pts, t), hip.flow(pts.to(DEV), t.to(DEV))
    assert scale_err(f["forward"].float(), f_ref["forward"]) < 1e-3 and scale_err(f["backward"].float(), f_ref["backward"]) < 1e-3
    dirs = torch.nn.functional.normalize(det_uniform((3000, 3), "adir", -1, 1), dim=-1)
    geo = det_uniform((3000, 15), "ageo", -1, 1)
    for m in (torch.zeros(3000, dtype=torch.bool), det_uniform((3000,), "am", 0, 1) > 0.8, torch.ones(3000, dtype=torch.bool)):
        a_ref = ref.attribute(pts, dirs, mask=m, geo_feat=geo)
        a = hip.attribute(pts.to(DEV), dirs.to(DEV), mask=m.to(DEV), geo_feat=geo.to(DEV).half())
        assert a.shape == (3000, 2) and a.dtype == torch.float32
        assert float((a.cpu() - a_ref).abs().max()) < 1e-3  # sigmoid outputs in [0, 1], fp16-rounded: two ulps at most


# ---- i. training ------------------------------------------------------------------------------------------------------------
def test_mixed_width_training_eager_and_graphed(monkeypatch):
    """Trainer on the synthetic dataset with LiDAR4D(hidden_dim_sigma=32, hidden_dim_lidar=128, hidden_dim_flow=16): two eager
    steps and two captured steps from identical state.  Finite losses, every network's parameters move, and the captured step
    agrees with the eager one as tests/test_gpu_optim.py::test_graph_replay_equals_eager_step asks of the default model
    (gradients to 1e-3 of each tensor's largest value, fewer than 1e-4 of the parameters off by more than 1e-4)."""
    from lidar4d_amd import LiDAR4D, trainer as trainer_mod
    from lidar4d_amd.data import SyntheticKitti360
    from lidar4d_amd.params import bump_epoch
    from lidar4d_amd.trainer import Trainer
    torch.manual_seed(0)
    m = LiDAR4D(**dict(SMALL_MODEL, **MIXED[0])).to(DEV)
    data = SyntheticKitti360(DEV, W=1024, num_rays=1024, seed=7, frame_seed=7)
    tr = Trainer(m, data, iters=200, chamfer=True, flow=True, ema_decay=None, init_scale=1024.0, graph_batch_inside=False)
    assert tr.graphs_supported()
    st, opt = m._store, tr.opt
    batch = {k: (v.contiguous().clone() if torch.is_tensor(v) else v) for k, v in data.batch_for(20).items()}
    monkeypatch.setattr(data, "batch_for", lambda frame: batch)
    render = m.render
    monkeypatch.setattr(m, "render", lambda *a, **kw: render(*a, **{**kw, "perturb": False}))
    tg, fl = torch.tensor([0.37], device=DEV), trainer_mod.flow_loss
    monkeypatch.setattr(trainer_mod, "flow_loss", lambda *a, **kw: fl(*a, **{**kw, "t_ground": tg}))
    for _ in range(4):  # let the loss scale settle
        assert np.isfinite(float(tr.train_step(batch)))
    opt.device_schedule()
    snap = {"flat": st.flat.detach().clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(), "steps": opt.steps.clone(),
            "scaler": tr.scaler.state.clone(), "sched": opt.sched.clone(), "count": opt.step_count}

    def restore():
        with torch.no_grad():
            st.flat.copy_(snap["flat"]), opt.exp_avg.copy_(snap["m"]), opt.exp_avg_sq.copy_(snap["v"]), opt.steps.copy_(snap["steps"])
            tr.scaler.state.copy_(snap["scaler"]), opt.sched.copy_(snap["sched"])
        opt.step_count = snap["count"]
        bump_epoch()
        st.refresh16()

    nets = {"flow_net": m.flow_net, "sigma_net": m.sigma_net, "intensity_net": m.intensity_net, "raydrop_net": m.raydrop_net}
    eager = []
    restore()
    for k in range(2):
        before = {n: [p.detach().clone() for p in net.parameters()] for n, net in nets.items()}
        loss = float(tr.train_step(batch))
        assert np.isfinite(loss) and bool(torch.isfinite(st.flat_grad).all())
        for n, net in nets.items():
            assert any(not torch.equal(a, b) for a, b in zip(before[n], net.parameters())), f"eager step {k}: {n} did not move"
        eager.append((loss, st.flat_grad.detach().clone(), st.flat.detach().clone()))
    restore()
    tr.train_step_graphed(20)  # eager warm-up + capture
    restore()
    for k in range(2):
        loss = float(tr.train_step_graphed(20))
        l_e, g_e, p_e = eager[k]
        assert np.isfinite(loss) and abs(loss - l_e) <= 1e-3 * abs(l_e), (k, loss, l_e)
        for name, p, off, n, gi in st.entries:
            if not n:
                continue
            a, b = st.flat_grad[off:off + n], g_e[off:off + n]
            assert bool(torch.isfinite(a).all()), f"replay {k}: non-finite gradient in {name}"
            d = float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)
            assert d < 1e-3, f"replay {k}: gradient of {name} differs from the eager step's by {d:.2e} of its largest value"
        off_frac = float(((st.flat - p_e).abs() > 1e-4).float().mean())
        assert off_frac < 1e-4, f"replay {k}: {off_frac:.2e} of the parameters differ from the eager step's"
    assert "liblidar4d_mlp" in open("/proc/self/maps").read()


# ---- j. the default widths never enter the new library ----------------------------------------------------------------------
_DEFAULT_RENDER = """
import sys, torch
sys.path.insert(0, {root!r})
from lidar4d_amd import LiDAR4D
from oracle.detparams import det_uniform, fill_model
from oracle.make_golden import SMALL_MODEL, test_rays
m = fill_model(LiDAR4D(**dict(SMALL_MODEL, density_scale=30.0)), seed=5).to("cuda")
ro, rd = test_rays(48, 3)
noise = det_uniform((48, 128), "vn", 0.0, 1.0)
o = m.render(ro.cuda(), rd.cuda(), torch.tensor([[0.5]]).cuda(), num_steps=128, perturb=True, noise=noise.cuda())
(o["depth_lidar"].sum() + o["image_lidar"].sum()).backward()
torch.cuda.synchronize()
torch.save({{"depth": o["depth_lidar"].detach().cpu(), "image": o["image_lidar"].detach().cpu(), "weights": o["weights"].detach().cpu(),
            "g_hash": m.hash_encoder.hash_static.params.grad.cpu()}}, {out!r})
mapped = "liblidar4d_mlp" in open("/proc/self/maps").read()
print("MAPPED" if mapped else "NOT MAPPED", "lidar4d_amd._mlp_lib" in sys.modules)
"""


def test_default_widths_never_map_the_library(tmp_path):
    """A model of the default widths renders and back-propagates in a fresh process without liblidar4d_mlp.so ever being mapped,
    and gives the bits this process gives with the library mapped: width 64 takes no part in the new code."""
    from lidar4d_amd import LiDAR4D, _mlp_lib
    out = str(tmp_path / "default.pt")
    res = subprocess.run([sys.executable, "-c", _DEFAULT_RENDER.format(root=ROOT, out=out)], capture_output=True, text=True, cwd=ROOT,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.strip().splitlines()[-1] == "NOT MAPPED False", res.stdout
    _mlp_lib.lib()
    assert "liblidar4d_mlp" in open("/proc/self/maps").read()
    m = fill_model(LiDAR4D(**dict(SMALL_MODEL, density_scale=30.0)), seed=5).to(DEV)
    ro, rd = make_rays(48, 3)
    noise = det_uniform((48, 128), "vn", 0.0, 1.0)
    o = m.render(ro.to(DEV), rd.to(DEV), torch.tensor([[0.5]]).to(DEV), num_steps=128, perturb=True, noise=noise.to(DEV))
    theirs = torch.load(out)
    for k, v in (("depth", o["depth_lidar"]), ("image", o["image_lidar"]), ("weights", o["weights"])):
        assert torch.equal(v.detach().cpu(), theirs[k]), k
    assert float(theirs["g_hash"].abs().sum()) > 0
