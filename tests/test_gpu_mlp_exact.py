"""The fused MLP kernels (csrc/mlp.hip) against a float64 reference on inputs for which every product, every sum in any order
and every fp16 / fp32 rounding is exact (tests/mlp_exact_ref.py): every comparison is torch.equal, no tolerance anywhere.
All 24 (in_pad, n_hidden) instantiations, ragged row counts, the device row count, the grid-stride loop, the caller's state
(grad_w accumulation, dx == null, sentinels past the end), dx_absmax, the ReLU gate at +-0, and the attribute networks whose
input rows are assembled in the kernel.  Run with ``-m gpu`` on an MI355X."""
import numpy as np
import pytest
import torch

import mlp_exact_ref as mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A  # bit pattern of rows the kernels must leave alone (as fp16: 203.25, a value that would open a ReLU gate)
EDGE_SHAPES = [(16, 2), (96, 2), (192, 3)]  # the narrow two-waves kernel, the prefetching kernel, the wide two-launch kernel
SIGMA_SHAPES = [(128, 1), (176, 2), (64, 1), (32, 2)]  # the widths the model configs run l4d_mlp_fwd_sigma at
LARGE_P = 131109


def ops_():
    from lidar4d_amd import ops
    return ops


def sent16(*shape):
    return torch.full(shape, SENT, dtype=torch.int16, device=DEV).view(torch.float16)


def untouched(t):
    return bool((t.view(torch.int16) == SENT).all())


def eq16(got, ref):
    got = got.cpu()
    return got.dtype == torch.float16 and torch.equal(got, mx.t16(ref))


def eq32(got, ref):
    got = got.cpu()
    return got.dtype == torch.float32 and torch.equal(got, mx.t32(ref))


def with_nan_past(a, n):
    """fp16 device copy of the lattice array whose rows from n on are NaN: rows the kernels may not look at."""
    t = mx.t16(a).clone()
    t[n:] = float("nan")
    return t.to(DEV)


def fwd_bwd_equal(c, x, w, dy, inv=1.0):
    """One forward and one backward on the whole case; everything equal to the reference.  -> the saved activations."""
    ops = ops_()
    y, act = ops.mlp_fwd(x, w, c.n_hidden, save_act=True)
    assert eq16(y, c.y), "y"
    assert eq16(act, c.act), "act"
    g = torch.zeros(w.numel(), device=DEV)
    dx = ops.mlp_bwd(x, act, dy, w, c.n_hidden, g, inv)
    assert eq16(dx, c.dx), "dx"
    assert eq32(g, c.grad(None, inv)), "grad_w"
    if ops.mlp_recompute_supported(c.in_pad, c.n_hidden):
        y2, none = ops.mlp_fwd(x, w, c.n_hidden, save_act=False)
        assert none is None and eq16(y2, c.y), "y (no activations stored)"
        g = torch.zeros(w.numel(), device=DEV)
        dx = ops.mlp_bwd(x, None, dy, w, c.n_hidden, g, inv)
        assert eq16(dx, c.dx), "dx (recomputed activations)"
        assert eq32(g, c.grad(None, inv)), "grad_w (recomputed activations)"
    return act


# ---- a. all 24 shapes, ragged rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [131, 33])
@pytest.mark.parametrize("in_pad,n_hidden", mx.SHAPES)
def test_every_shape_equals_float64(in_pad, n_hidden, P):
    ops = ops_()
    c = mx.case(in_pad, n_hidden, P)
    c.stats_ok()
    x, w, dy = mx.t16(c.x).to(DEV), c.w16().to(DEV), mx.t16(c.dy).to(DEV)
    fwd_bwd_equal(c, x, w, dy)
    if (in_pad, n_hidden) in SIGMA_SHAPES:
        y, act, sigma = ops.mlp_fwd_sigma(x, w, n_hidden, save_act=True)
        assert eq16(y, c.y) and eq16(act, c.act)
        assert sigma.shape == (P,)


def test_recompute_covers_the_documented_shapes():
    ops = ops_()
    got = {s for s in mx.SHAPES if ops.mlp_recompute_supported(*s)}
    assert got == {s for s in mx.SHAPES if s[0] <= 32} | {(128, 1)}


# ---- b. row-count edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 15, 16, 17, 31, 32, 33, 63, 65])
@pytest.mark.parametrize("in_pad,n_hidden", EDGE_SHAPES)
def test_row_count_edges(in_pad, n_hidden, P):
    ops = ops_()
    c = mx.case(in_pad, n_hidden, P)
    w = c.w16().to(DEV)
    fwd_bwd_equal(c, mx.t16(c.x).to(DEV), w, mx.t16(c.dy).to(DEV))
    for n in sorted({0, 1, P - 1, P, P + 100}):
        m = min(n, P)
        n_rows = torch.tensor([n], dtype=torch.int32, device=DEV)
        x, dy = with_nan_past(c.x, m), with_nan_past(c.dy, m)
        y, act, dx = sent16(P, 16), sent16(n_hidden, P, 64), sent16(P, in_pad)
        ops.mlp_fwd(x, w, n_hidden, save_act=True, n_rows=n_rows, y=y, act=act)
        assert eq16(y[:m], c.y[:m]) and eq16(act[:, :m], c.act[:, :m]), (n, "forward")
        assert untouched(y[m:]) and untouched(act[:, m:]), (n, "forward wrote past the row count")
        paths = [act] + ([None] if ops.mlp_recompute_supported(in_pad, n_hidden) else [])
        for a in paths:
            dx.view(torch.int16).fill_(SENT)
            g = torch.full((w.numel(),), 3.0, device=DEV)
            ops.mlp_bwd(x, a, dy, w, n_hidden, g, 1.0, n_rows=n_rows, dx=dx)
            assert eq16(dx[:m], c.dx[:m]), (n, a is None, "dx")
            assert untouched(dx[m:]), (n, a is None, "backward wrote past the row count")
            assert eq32(g, c.grad(m) + 3.0), (n, a is None, "grad_w")  # n = 0: unchanged


# ---- c. grid-stride loop and prefetch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_pad,n_hidden", EDGE_SHAPES)
def test_grid_stride_and_prefetch(in_pad, n_hidden):
    """131,109 rows: more than one forward sweep (2048 x 4 x 16 rows) and more than two backward sweeps of the narrow kernel at
    256 CUs, so waves take several tiles, prefetch across them, clamp past the end, and the last tile is ragged."""
    c = mx.case(in_pad, n_hidden, LARGE_P, amp=1)
    c.stats_ok()
    fwd_bwd_equal(c, mx.t16(c.x).to(DEV), c.w16().to(DEV), mx.t16(c.dy).to(DEV), inv=1.0 / 128)


# ---- d. the caller's state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_pad,n_hidden", EDGE_SHAPES)
def test_grad_w_accumulates_into_callers_state(in_pad, n_hidden):
    ops = ops_()
    c = mx.case(in_pad, n_hidden, 131)
    x, w, dy = mx.t16(c.x).to(DEV), c.w16().to(DEV), mx.t16(c.dy).to(DEV)
    _, act = ops.mlp_fwd(x, w, n_hidden, save_act=True)
    prefill = mx.lattice_ints((w.numel(),), 3, (in_pad, n_hidden, 7))
    for inv in (1.0, 1.0 / 128):
        g = mx.t32(prefill).to(DEV)
        dx = ops.mlp_bwd(x, act, dy, w, n_hidden, g, inv)
        assert eq16(dx, c.dx) and eq32(g, prefill + c.grad(None, inv)), inv
        g2 = mx.t32(prefill).to(DEV)
        assert ops.mlp_bwd(x, act, dy, w, n_hidden, g2, inv, want_dx=False) is None
        assert torch.equal(g2, g), (inv, "dx == null changes grad_w")
        g3 = torch.zeros(w.numel(), device=DEV)
        ops.mlp_bwd(x, act, dy, w, n_hidden, g3, inv)
        ops.mlp_bwd(x, act, dy, w, n_hidden, g3, inv, want_dx=False)
        assert eq32(g3, 2.0 * c.grad(None, inv)), (inv, "two calls into one grad_w")


# ---- e. dx_absmax -----------------------------------------------------------------------------------------------------------
ABSMAX_TILE_SCALE = {1: 4.0, 3: 16.0, 5: 8.0, 7: 4.0, 9: 4.0}  # W1's odd 16-column tiles; the even ones keep +-1


def absmax_case(in_pad, n_hidden, P):
    """The lattice with the odd 16-column tiles of W1 scaled by powers of two: every even tile then has a larger |dx| in both
    neighbours, so a column range that is one tile too wide at either end gives a wrong number, and the multi-tile ranges
    differ in their maxima (both asserted by the test)."""
    Ws = mx.lattice_weights(in_pad, n_hidden)
    for tile, f in ABSMAX_TILE_SCALE.items():
        Ws[0][:, 16 * tile:16 * tile + 16] *= f
    return mx.Case(in_pad, n_hidden, P, Ws=Ws)


@pytest.mark.parametrize("in_pad,n_hidden,ranges", [(128, 1, [(0, 16), (64, 128), (0, 128)]),
                                                    (176, 2, [(0, 16), (64, 128), (0, 176), (96, 176)])])
def test_dx_absmax(in_pad, n_hidden, ranges):
    ops = ops_()
    P, n = 131, 77
    c = absmax_case(in_pad, n_hidden, P)
    wants = [float(np.abs(c.dx[:, lo:hi]).max()) for lo, hi in ranges]
    assert len(set(wants)) == len(wants), ("every range has a maximum of its own", wants)
    tile_max = [float(np.abs(c.dx[:, 16 * t:16 * t + 16]).max()) for t in range(in_pad // 16)]
    for t in range(0, in_pad // 16, 2):  # an even tile alone: one tile too many at either end raises the maximum
        assert all(tile_max[u] > tile_max[t] > 0 for u in (t - 1, t + 1) if 0 <= u < in_pad // 16), tile_max
    ranges = ranges + [(16 * t, 16 * t + 16) for t in range(in_pad // 16) if (16 * t, 16 * t + 16) not in ranges]
    x, w, dy = mx.t16(c.x).to(DEV), c.w16().to(DEV), mx.t16(c.dy).to(DEV)
    _, act = ops.mlp_fwd(x, w, n_hidden, save_act=True)
    paths = [act] + ([None] if ops.mlp_recompute_supported(in_pad, n_hidden) else [])
    g = torch.zeros(w.numel(), device=DEV)
    n_rows = torch.tensor([n], dtype=torch.int32, device=DEV)
    x_n, dy_n = with_nan_past(c.x, n), with_nan_past(c.dy, n)
    live = int(np.argmax((c.act > 0).sum(2).min(0)))  # a row with active units in every layer: an inf in its dy reaches dx
    assert (c.act[:, live] > 0).any(1).all()
    dy_inf = dy.clone()
    dy_inf[live, 3] = float("inf")
    for a in paths:
        for lo, hi in ranges:
            want = float(np.abs(c.dx[:, lo:hi]).max())
            assert want > 0
            amax = torch.zeros(1, device=DEV)
            dx = ops.mlp_bwd(x, a, dy, w, n_hidden, g, 1.0, dx_absmax=amax, absmax_cols=(lo, hi))
            assert eq16(dx, c.dx) and float(amax) == want, (lo, hi, float(amax), want)
            big = torch.full((1,), want + 0.5, device=DEV)  # a larger value already there is kept
            ops.mlp_bwd(x, a, dy, w, n_hidden, g, 1.0, dx_absmax=big, absmax_cols=(lo, hi))
            assert float(big) == want + 0.5
            small = torch.full((1,), 0.25, device=DEV)  # a smaller one is raised
            ops.mlp_bwd(x, a, dy, w, n_hidden, g, 1.0, dx_absmax=small, absmax_cols=(lo, hi))
            assert float(small) == want
            want_n = float(np.abs(c.dx[:n, lo:hi]).max())  # rows past the device row count do not count
            amax = torch.zeros(1, device=DEV)
            ops.mlp_bwd(x_n, a, dy_n, w, n_hidden, g, 1.0, n_rows=n_rows, dx_absmax=amax, absmax_cols=(lo, hi))
            assert float(amax) == want_n, (lo, hi, float(amax), want_n)
            amax = torch.zeros(1, device=DEV)
            ops.mlp_bwd(x, a, dy_inf, w, n_hidden, torch.zeros_like(g), 1.0, dx_absmax=amax, absmax_cols=(lo, hi))
            assert float(amax) == float("inf"), (lo, hi, float(amax))
    from lidar4d_amd._lib import HipExtensionError
    amax = torch.zeros(1, device=DEV)
    for bad in ((8, 32), (0, 24), (0, in_pad + 16), (-16, 16)):
        with pytest.raises(HipExtensionError, match="dx_absmax needs dx and a column range"):
            ops.mlp_bwd(x, act, dy, w, n_hidden, g, 1.0, dx_absmax=amax, absmax_cols=bad)
    with pytest.raises(HipExtensionError, match="dx_absmax needs dx and a column range"):
        ops.mlp_bwd(x, act, dy, w, n_hidden, g, 1.0, want_dx=False, dx_absmax=amax, absmax_cols=ranges[0])
    assert float(amax) == 0.0


# ---- f. the ReLU gate at +-0 ------------------------------------------------------------------------------------------------
TINY = 2.0 ** -13  # a normal fp16 number whose square, 2^-26, is below half the smallest fp16 subnormal: it rounds to (+-)0
KINDS = ("neg_tiny", "pos_tiny", "zero", "pos", "neg")  # pre-activation -2^-26, +2^-26, exactly 0, +3, -3
GATE_ROWS = (0, 13, 37, 69)  # the rows that carry anything: both halves of a 32-row macro tile, three tiles, the ragged last row


def kind_of(m):
    return KINDS[m % 5]  # neighbours differ: the packed fp16 pairs mix a -0 with every other kind


def gate_problem(n_hidden):
    """x [70, 16] (zero but for GATE_ROWS: column 0 = 2^-13, columns 1, 2 = 3), weights that put every hidden unit of the gated
    layer(s) into one of KINDS, dy = 1 and an output layer that hands every unit of the last hidden layer dh = 1."""
    P = 70
    x = np.zeros((P, 16))
    x[list(GATE_ROWS), 0], x[list(GATE_ROWS), 1], x[list(GATE_ROWS), 2] = TINY, 3.0, 3.0
    carrier = 40  # (n_hidden = 2) the layer-1 unit whose activation is 2^-13: the tiny products of layer 2 come from it
    W1 = np.zeros((64, 16))
    kinds1 = []
    for m in range(64):
        k = "carrier" if (n_hidden == 2 and m == carrier) else kind_of(m)
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
        pos1 = [m for m in range(64) if kinds1[m] == "pos"]
        dead1 = [m for m in range(64) if kinds1[m] in ("neg_tiny", "pos_tiny", "zero", "neg")]
        W2 = np.zeros((64, 64))
        for m in range(64):
            k = kind_of(m)
            if k == "neg_tiny":
                W2[m, carrier] = -TINY
            elif k == "pos_tiny":
                W2[m, carrier] = TINY
            elif k == "zero":
                W2[m, pos1[0]], W2[m, pos1[1]] = 1.0, -1.0
            elif k == "pos":
                W2[m, pos1[m % len(pos1)]] = 1.0
                W2[m, dead1] = 1.0  # a dead layer-1 unit adds nothing forward, and receives dh1 > 0: a leak would show
            else:
                W2[m, pos1[m % len(pos1)]] = -1.0
        Ws.append(W2)
        kinds.append([kind_of(m) for m in range(64)])
    Wo = np.zeros((16, 64))
    Wo[np.arange(64) % 16, np.arange(64)] = 1.0
    Ws.append(Wo)
    return x, np.ones((P, 16)), Ws, kinds


@pytest.mark.parametrize("n_hidden", [1, 2])
def test_relu_gate_at_signed_zero(n_hidden):
    """A pre-activation of -2^-26 rounds to fp16 -0.  The stored activation must be +0 (l4d_mlp_bwd's gate opens on a non-zero
    bit pattern), and no gradient may pass a unit at +-2^-26 or at 0, with saved and with recomputed activations."""
    ops = ops_()
    x64, dy64, Ws, kinds = gate_problem(n_hidden)
    y_ref, act_ref = mx.forward(x64, Ws, strict=False)
    dx_ref, dW_ref = mx.backward(x64, act_ref, dy64, Ws, strict=False)
    P = x64.shape[0]
    special = np.zeros(P, dtype=bool)
    special[list(GATE_ROWS)] = True
    for l in range(n_hidden):  # the reference itself: a unit is active exactly on the special rows, and only if "pos"/"carrier"
        for m in range(64):
            on = kinds[l][m] in ("pos", "carrier")
            assert ((act_ref[l][:, m] > 0) == (special & on)).all()
    assert (dx_ref[~special] == 0).all() and (dx_ref[special] != 0).any()
    x, w, dy = mx.t16(x64).to(DEV), torch.from_numpy(mx.pack(Ws)).to(DEV), mx.t16(dy64).to(DEV)
    y, act = ops.mlp_fwd(x, w, n_hidden, save_act=True)
    bits = act.view(torch.int16).cpu()
    assert bool((bits >= 0).all()), f"{int((bits < 0).sum())} stored activations carry a sign bit (-0)"
    assert eq16(y, y_ref) and eq16(act, act_ref)
    assert np.array_equal(act.cpu().numpy() > 0, act_ref > 0)
    assert ops.mlp_recompute_supported(16, n_hidden)
    for a in (act, None):
        g = torch.zeros(w.numel(), device=DEV)
        dx = ops.mlp_bwd(x, a, dy, w, n_hidden, g, 1.0)
        assert eq16(dx, dx_ref), ("dx", a is None)
        assert eq32(g, dW_ref), ("grad_w", a is None)
        g, off = g.cpu().numpy(), 0
        for l in range(n_hidden):  # dW_l[m, :] shows unit m's gate alone: gradient reaches it iff the stored activation is > 0
            cols = Ws[l].shape[1]
            dWl = g[off:off + 64 * cols].reshape(64, cols)
            off += 64 * cols
            for m in range(64):
                if kinds[l][m] == "pos":  # (the carrier is active, but feeds only units at +-2^-26: nothing comes back to it)
                    assert dWl[m].any(), (l, m, kinds[l][m], a is None)
                else:
                    assert not dWl[m].any(), (l, m, kinds[l][m], a is None, "gradient through a dead unit")
        assert not dx.cpu()[torch.from_numpy(~special)].any()


# ---- g. the attribute networks on the lattice -------------------------------------------------------------------------------
def attr_problem():
    n_rays, T, n_enc, n_geo, in_pad = 37, 64, 72, 15, 96
    P = n_rays * T
    denc = mx.lattice_ints((n_rays, n_enc), 2, (96, 1))
    h = mx.lattice_ints((P, 16), 2, (96, 2))
    rng = np.random.RandomState(5)
    keep = np.nonzero(rng.rand(P - 1) < 0.5)[0]
    idx = np.concatenate([[P - 1], rng.permutation(keep)]).astype(np.int32)  # shuffled; first: the last sample of the last ray
    M = idx.size
    rows = np.concatenate([denc[idx // T], h[idx, 1:1 + n_geo], np.ones((M, in_pad - n_enc - n_geo))], 1)  # logical order
    phys = np.concatenate([rows[:, :n_enc], np.ones((M, 1)), rows[:, n_enc:n_enc + n_geo], np.ones((M, 8))], 1)
    dy = mx.lattice_ints((P, 16), 2, (96, 3))
    return dict(n_rays=n_rays, T=T, n_enc=n_enc, n_geo=n_geo, in_pad=in_pad, P=P, M=M, denc=denc, h=h, idx=idx, rows=rows,
                phys=phys, dy=dy)


@pytest.fixture(scope="module")
def attr():
    return attr_problem()


@pytest.mark.parametrize("n_hidden", [1, 2, 3])
def test_attr_networks_equal_float64(attr, n_hidden):
    ops = ops_()
    A = attr
    P, M, T, in_pad, n_enc, n_geo = A["P"], A["M"], A["T"], A["in_pad"], A["n_enc"], A["n_geo"]
    assert ops.attr_mlp_supported(in_pad, n_enc, n_geo) and 33 < M < P
    c = mx.Case(in_pad, n_hidden, M, x=A["rows"], dy=A["dy"][:M].copy(), Ws=mx.lattice_weights(in_pad, n_hidden, seed=3))
    c.stats_ok()
    w = c.w16().to(DEV)
    denc, h = mx.t16(A["denc"]).to(DEV), mx.t16(A["h"]).to(DEV)
    idx = torch.zeros(P, dtype=torch.int32, device=DEV)
    idx[:M] = torch.from_numpy(A["idx"]).to(DEV)
    for n in (0, 1, 17, 33, M):
        count = torch.tensor([n], dtype=torch.int32, device=DEV)
        xr = sent16(P, in_pad)
        y, act = ops.attr_mlp_fwd(idx, count, P, T, denc, h, n_geo, in_pad, w, n_hidden, save_act=True, x_rows_out=xr)
        assert eq16(y[:n], c.y[:n]) and eq16(act[:, :n], c.act[:, :n]), (n, "forward")
        assert eq16(xr[:n], A["phys"][:n]) and untouched(xr[n:]), (n, "stored rows")
        y2, none = ops.attr_mlp_fwd(idx, count, P, T, denc, h, n_geo, in_pad, w, n_hidden, save_act=False)
        assert none is None and eq16(y2[:n], c.y[:n])
        dy = with_nan_past(A["dy"], n)
        tails = []
        g = torch.full((w.numel(),), 3.0, device=DEV)
        tails.append(("stored rows", ops.attr_mlp_bwd(xr, count, n_enc, n_geo, act, dy, w, n_hidden, g, 1.0 / 128), g))
        if ops.attr_mlp_bwd_gathered_supported(n_hidden):
            g = torch.full((w.numel(),), 3.0, device=DEV)
            tails.append(("gathered", ops.attr_mlp_bwd_gathered(idx, count, P, T, denc, h, n_geo, in_pad, act, dy, w, n_hidden, g,
                                                                1.0 / 128), g))
        else:
            assert n_hidden == 3
        for what, tail, g in tails:
            assert tail.shape == (P, in_pad - 64)
            # dx_tail = physical columns 64 .. 95: [64 .. 71 | d/d(one), g0 .. g14 | 88 .. 95]
            assert eq16(tail[:n, 0:8], c.dx[:n, 64:72]), (n, what, "dx 64..71")
            assert eq16(tail[:n, 9:24], c.dx[:n, 72:87]), (n, what, "dx g0..g14")
            assert eq16(tail[:n, 24:32], c.dx[:n, 88:96]), (n, what, "dx 88..95")
            assert eq32(g, c.grad(n, 1.0 / 128) + 3.0), (n, what, "grad_w in the logical column order")
