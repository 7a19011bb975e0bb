"""Exact tests of the hash-grid kernels (csrc/hashgrid.hip, csrc/hashgrid_dev.h) and of the sorted gradient scatter (csrc/binscatter.hip)
through lidar4d_amd.ops, against the float64 references of tests/hashgrid_cases.py (whose header says why the comparisons can be
bit for bit, and derives the bound of the sorted scatter).  Every result is compared by its bits; only the binned levels of the sorted
scatter have a bound.  Run with ``-m gpu`` on an MI355X."""
import numpy as np
import pytest
import torch

import hashgrid_cases as hc
from hashgrid_cases import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F32, F64 = np.float16, np.float32, np.float64
SENT16, SENT32 = F16(-77.0), F32(-77.0)
DENSE = hc.COORD_LAYOUTS[0]


def T(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def meta_of(geom):
    from lidar4d_amd.gridmeta import GridMeta
    return GridMeta(*geom.grid_meta_args())


def coords_tensor(x, layout=DENSE):
    """-> (tensor [P, width], cols): the unused columns are NaN; ``row4_misaligned`` starts one float into its buffer."""
    name, width, cols, misaligned = layout
    P, D = x.shape
    if width is None:
        return T(x), tuple(range(D))
    cols = cols[:D]
    arr = hc.place(x, width, cols)
    if not misaligned:
        t = T(arr)
        assert t.data_ptr() % 16 == 0
        return t, cols
    buf = torch.full((arr.size + 1,), float("nan"), dtype=torch.float32, device=DEV)
    buf[1:] = T(arr.ravel())
    t = buf[1:].view(P, width)
    assert (P == 0 or t.data_ptr() % 16 == 4) and t.is_contiguous()
    return t, cols


def wide(values, stride, col, sentinel, extra_rows=0):
    """values [P, w] placed at column ``col`` of rows of ``stride`` elements, ``sentinel`` everywhere else (and in extra rows)."""
    out = np.full((values.shape[0] + extra_rows, stride), sentinel, values.dtype)
    out[:values.shape[0], col:col + values.shape[1]] = values
    return out


def assert_bits(got, want, what):
    eq = same_bits(got, want)
    bad = np.flatnonzero(~eq.reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {eq.size} values differ, first at {bad[:5]}: got {got.reshape(-1)[bad[:5]]}, "
                           f"want {want.reshape(-1)[bad[:5]]}")


def t_dev(t):
    return torch.tensor([t], dtype=torch.float32, device=DEV)


# ---- forward (class L) --------------------------------------------------------------------------------------------------------------
def run_fwd(c, layout=DENSE, out_col=0, stride=None, level_major=None):
    from lidar4d_amd import ops
    geom = c["geom"]
    P, W = c["x"].shape[0], geom.n_output_dims
    stride = W if stride is None else stride
    x, cols = coords_tensor(c["x"], layout)
    want = wide(c["out16"], stride, out_col, SENT16, extra_rows=3)  # P = 0 and the rows behind P: untouched
    out = T(np.full_like(want, SENT16))
    ops.hashgrid_fwd(meta_of(geom), x, cols, T(c["table"]), out=out, out_col=out_col, level_major=level_major)
    torch.cuda.synchronize()
    return N(out), want


@pytest.mark.parametrize("D,F", hc.DF)
def test_forward_every_point_count(D, F):
    """The default route of ops.hashgrid_fwd: one thread per (point, level) below 4096 points, hashgrid_fwd_rows_kernel from there on
    (for F = 2 the six levels are 12 columns, no multiple of 8: the first kernel at every size -- see the four-level case below)."""
    for P in hc.POINT_COUNTS:
        got, want = run_fwd(hc.fwd_case(D, F, P))
        assert_bits(got, want, f"hashgrid_fwd D={D} F={F} P={P}")


@pytest.mark.parametrize("D,F", hc.DF)
def test_forward_level_major(D, F):
    """level_major=True: hashgrid_fwd_levels_kernel (with the x-neighbour pair loads for F = 4) and hashgrid_rows_from_levels_kernel."""
    for P in (0, 1, 65, 257, 4159):
        got, want = run_fwd(hc.fwd_case(D, F, P), level_major=True)
        assert_bits(got, want, f"hashgrid_fwd level-major D={D} F={F} P={P}")


@pytest.mark.parametrize("P", [4095, 4096, 4159])
def test_forward_rows_kernel_two_features(P):
    """F = 2 with four levels (8 columns): the only F = 2 shape the row kernels take."""
    c = hc.fwd_case(3, 2, P, 4)
    for lm in (None, True):
        got, want = run_fwd(c, level_major=lm)
        assert_bits(got, want, f"hashgrid_fwd D=3 F=2 L=4 P={P} level_major={lm}")


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("layout", hc.COORD_LAYOUTS[1:], ids=[l[0] for l in hc.COORD_LAYOUTS[1:]])
def test_forward_coordinate_layouts(D, layout):
    """Rows of 4 floats (aligned: the float4 load of load_coords_nt; one float into the buffer: the scalar path), rows of 5 with
    permuted columns; NaN in every column that must not be read."""
    for F, P, lm in ((4, 257, None), (4, 257, True), (8, 4159, None), (8, 4159, True), (2, 65, None)):
        got, want = run_fwd(hc.fwd_case(D, F, P), layout=layout, level_major=lm)
        assert_bits(got, want, f"hashgrid_fwd {layout[0]} D={D} F={F} P={P} level_major={lm}")


@pytest.mark.parametrize("D,F", [(3, 4), (2, 8), (3, 2)])
def test_forward_into_a_wider_row(D, F):
    """out_col > 0 in a wider row (multiples of F: the kernels store an entry's F halfs as one vector): 16-byte aligned with a row
    stride of a multiple of 8 (row kernels), and not (the per-level kernel at every size); the columns outside keep their bits."""
    W = 6 * F
    for P in (257, 4159):
        for out_col, stride, lm in ((8, W + 16, None), (8, W + 16, True), (F, W + 2 * F, None), (F, W + 3 * F, True)):
            got, want = run_fwd(hc.fwd_case(D, F, P), out_col=out_col, stride=stride, level_major=lm)
            assert_bits(got, want, f"hashgrid_fwd D={D} F={F} P={P} out_col={out_col} stride={stride} level_major={lm}")


# ---- backward (class L) -------------------------------------------------------------------------------------------------------------
def run_bwd(c, grad_scale, half, layout=DENSE, dout_col=0, stride=None):
    from lidar4d_amd import ops
    geom = c["geom"]
    W = geom.n_output_dims
    x, cols = coords_tensor(c["x"], layout)
    dt = F16 if half else F32
    dout = hc.to_f32_exact(c["dout"]).astype(dt)
    assert (dout.astype(F64) == c["dout"]).all()
    dout = wide(dout, W if stride is None else stride, dout_col, dt(np.nan), extra_rows=2)
    g = T(c["g0"])
    ops.hashgrid_bwd(meta_of(geom), x, cols, T(dout), g, grad_scale=grad_scale, dout_col=dout_col)
    torch.cuda.synchronize()
    return N(g)


@pytest.mark.parametrize("D,F", hc.DF)
def test_backward_every_point_count(D, F):
    """l4d_hashgrid_bwd: wave run reduction + fp32 atomics, fp16 and fp32 dout, every grad_scale, onto zeros and onto a prefilled table."""
    k = 0
    for P in hc.POINT_COUNTS:
        for half in (True, False):
            gs, pre = hc.GRAD_SCALES[k % 3], (k // 2) % 2 == 0
            k += 1
            c = hc.bwd_case(D, F, P, "scattered", gs, pre)
            assert_bits(run_bwd(c, gs, half), c["ref"], f"hashgrid_bwd D={D} F={F} P={P} half={half} grad_scale={gs} prefilled={pre}")


@pytest.mark.parametrize("D,F", hc.DF)
def test_backward_runs(D, F):
    """Runs of 1 .. 70 equal points across the wavefront and workgroup edges, rows without a gradient inside them, one wavefront
    without any, the last run ending at P - 1; and every point in one cell."""
    for P, kind, gs, pre in ((4159, "runs", 1.0, False), (257, "runs", 128.0, True), (255, "runs", 0.25, True), (257, "one_cell", 128.0, True)):
        c = hc.bwd_case(D, F, P, kind, gs, pre)
        for half in (True, False):
            assert_bits(run_bwd(c, gs, half), c["ref"], f"hashgrid_bwd {kind} D={D} F={F} P={P} half={half}")


@pytest.mark.parametrize("D", [2, 3])
def test_backward_layouts(D):
    """Coordinate layouts and dout_col > 0 in a wider row (NaN outside the columns that are read)."""
    c = hc.bwd_case(D, 4, 257, "scattered", 0.25, True)
    for i, layout in enumerate(hc.COORD_LAYOUTS):
        got = run_bwd(c, 0.25, half=i % 2 == 0, layout=layout, dout_col=(0, 8, 3, 5)[i], stride=24 + (0, 16, 5, 8)[i])
        assert_bits(got, c["ref"], f"hashgrid_bwd {layout[0]} D={D}")


@pytest.mark.parametrize("half", [True, False])
def test_backward_nonfinite_gradient_atomic_route(half):
    """One +inf in dout of level 4: that level's gradient holds a non-finite value (common.h, f2h_grad), the other levels stay bit-exact."""
    c = dict(hc.bwd_case(3, 4, 257, "scattered", 1.0, True))
    geom = c["geom"]
    c["dout"] = c["dout"].copy()
    c["dout"][100, 4 * 4 + 1] = np.inf
    from lidar4d_amd import ops
    x, cols = coords_tensor(c["x"])
    g = T(c["g0"])
    ops.hashgrid_bwd(meta_of(geom), x, cols, T(c["dout"].astype(F16 if half else F32)), g, grad_scale=1.0)
    got = N(g)
    for lvl in range(6):
        sl = geom.level_slice(lvl, 4)
        if lvl == 4:
            assert not np.isfinite(got[sl]).all()
            f1 = np.arange(sl.stop - sl.start) % 4 != 1  # the other features of the level never see the inf
            assert_bits(got[sl][f1], c["ref"][sl][f1], "other features of level 4")
        else:
            assert_bits(got[sl], c["ref"][sl], f"level {lvl}")


# ---- time-blended kernels (class E on exact slice features) -------------------------------------------------------------------------
@pytest.mark.parametrize("D,F", hc.DF_T)
@pytest.mark.parametrize("n_slices,t", hc.T_SETUPS)
def test_time_forward(D, F, n_slices, t):
    from lidar4d_amd import ops
    W = 6 * F // 4
    for i, P in enumerate(hc.POINT_COUNTS):
        c = hc.t_fwd_case(D, F, P, n_slices, t)
        meta = meta_of(c["geom"])
        tabs = [T(tb) for tb in c["tables"]]
        layout = hc.COORD_LAYOUTS[i % 4]
        x, cols = coords_tensor(c["x"], layout)
        for half_out, out_col, stride in ((False, 0, W), (True, 0, W), (False, 3, W + 5), (True, 8, W + 16)):
            ref = c["out32"].astype(F16) if half_out else c["out32"]
            want = wide(ref, stride, out_col, SENT16 if half_out else SENT32, extra_rows=2)
            out = T(np.full_like(want, want.dtype.type(-77.0)))
            ops.hashgrid_t_fwd(meta, x, cols, tabs, t_dev(t), out=out, out_col=out_col, half_out=half_out)
            assert_bits(N(out), want, f"hashgrid_t_fwd D={D} F={F} P={P} slices={n_slices} t={t} half={half_out} out_col={out_col} {layout[0]}")


@pytest.mark.parametrize("D,F", hc.DF_T)
@pytest.mark.parametrize("n_slices,t", hc.T_SETUPS)
def test_time_backward_atomic_route(D, F, n_slices, t):
    """l4d_hashgrid_t_bwd below the sorted scatter's threshold: Hs by run-reduced atomics (exact), then the expand kernel (class E) on
    top of prefilled slice gradients; the slices t does not select keep their bits."""
    from lidar4d_amd import ops
    W = 6 * F // 4
    cases = [(P, "scattered") for P in hc.POINT_COUNTS] + [(257, "runs"), (4159, "runs"), (257, "one_cell")]
    for i, (P, kind) in enumerate(cases):
        gs = hc.GRAD_SCALES[i % 3]
        c = hc.t_bwd_case(D, F, P, n_slices, t, kind, gs)
        assert P * (1 << D) < ops.BINNED_SCATTER_MIN_RECORDS
        x, cols = coords_tensor(c["x"], hc.COORD_LAYOUTS[(i + 1) % 4])
        half = i % 2 == 0
        dt = F16 if half else F32
        dout_col, stride = ((0, W), (8, W + 16), (3, W + 5))[i % 3]
        dout = wide(c["dout"].astype(dt), stride, dout_col, dt(np.nan), extra_rows=2)
        grads = [T(g) for g in c["grads0"]]
        ops.hashgrid_t_bwd(meta_of(c["geom"]), x, cols, n_slices, t_dev(t), T(dout), grads, grad_scale=gs, dout_col=dout_col)
        for s in range(n_slices):
            assert_bits(N(grads[s]), c["grads_ref"][s], f"hashgrid_t_bwd D={D} F={F} P={P} {kind} slices={n_slices} t={t} slice {s} half={half}")


def test_time_forward_level_major_threshold():
    """l4d_hashgrid_t_fwd_ws takes its level-major kernels from 2^18 points on (D = 3, F = 8, fp16 output, 4 levels = 8 columns):
    exactly 2^18 points through them, and the same inputs without the last point through the row kernel."""
    from lidar4d_amd import ops
    c = hc.t_fwd_big_case()
    meta = meta_of(c["geom"])
    assert ops.FLOW_LEVELS_MIN_POINTS == hc.LEVELS_MIN_POINTS == c["x"].shape[0]
    tabs = [T(tb) for tb in c["tables"]]
    x4, cols = coords_tensor(c["x"], hc.COORD_LAYOUTS[1])
    for P in (hc.LEVELS_MIN_POINTS, hc.LEVELS_MIN_POINTS - 1):
        want = wide(c["out16"][:P], 8, 0, SENT16, extra_rows=2)
        out = T(np.full_like(want, SENT16))
        ops.hashgrid_t_fwd(meta, x4[:P], cols, tabs, t_dev(c["t"]), out=out, half_out=True)
        assert_bits(N(out), want, f"hashgrid_t_fwd P={P}")


# ---- sorted scatter against float64 (class B) ---------------------------------------------------------------------------------------
def run_sorted(monkeypatch, r, g64, grad_scale, padded):
    """Hs of l4d_hashgrid_t_bwd's sorted route: one slice at t = 0, where the basis is exactly (1, 0, 0, 0) -- the first F / 4
    features of every entry receive Hs, the others nothing.  padded: dout at column 8 of 32-column rows (16-byte aligned pieces: the
    register window of bin_pass1_kernel); otherwise dense rows of 6 or 12 halfs (its other path)."""
    from lidar4d_amd import ops
    monkeypatch.setattr(ops, "BINNED_SCATTER_MIN_RECORDS", 1)
    geom = r["geom"]
    F, FO = geom.n_features, geom.n_features // 4
    x, cols = coords_tensor(r["x"], hc.COORD_LAYOUTS[1] if padded else DENSE)
    with np.errstate(invalid="ignore"):
        d16 = g64.astype(F16)
    dout = wide(d16, 32, 8, F16(np.nan)) if padded else d16
    g = torch.zeros(geom.n_entries * F, dtype=torch.float32, device=DEV)
    ops.hashgrid_t_bwd(meta_of(geom), x, cols, 1, t_dev(0.0), T(dout), [g], grad_scale=grad_scale, dout_col=8 if padded else 0)
    torch.cuda.synchronize()
    got = N(g).reshape(-1, F)
    clean = np.isfinite(got[:, :FO]).all(1)  # (a non-finite Hs times a basis value of 0 is NaN: handed on, as it must be)
    assert not got[clean, FO:].any(), "features of the basis functions that are zero at t = 0 received a gradient"
    return got[:, :FO].reshape(-1)


@pytest.mark.parametrize("D,F", hc.SCATTER_DF)
@pytest.mark.parametrize("P", hc.SCATTER_P)
@pytest.mark.parametrize("cloud", hc.SCATTER_CLOUDS)
def test_sorted_scatter_against_float64(monkeypatch, D, F, P, cloud):
    """bs_scatter at P = 2048 (grad_scale 1, dense dout rows) and 8192 (grad_scale 0.25, padded rows): dense levels bit-exact, binned
    levels within the bound derived in hashgrid_cases.py, element by element."""
    r = hc.scatter_case(D, F, P, cloud)
    geom, FO = r["geom"], F // 4
    gs = 1.0 if P == 2048 else 0.25
    got = run_sorted(monkeypatch, r, r["g"], gs, padded=P != 2048)
    ref, bound = r["ref"] * gs, r["bound"] * gs
    worst = 0.0
    for lvl, binned in enumerate(r["binned"]):
        sl = geom.level_slice(lvl, FO)
        if not binned:
            assert_bits(got[sl], hc.to_f32_exact(ref[sl]), f"dense level {lvl}")
            continue
        err = np.abs(got[sl].astype(F64) - ref[sl])
        bad = np.flatnonzero(err > bound[sl])
        worst = max(worst, float((err / np.maximum(bound[sl], 1e-300))[bound[sl] > 0].max(initial=0.0)))
        assert bad.size == 0, (f"binned level {lvl}: {bad.size} of {err.size} elements outside their bound, first at {bad[:5]}: got "
                               f"{got[sl][bad[:5]]}, want {ref[sl][bad[:5]]}, bound {bound[sl][bad[:5]]}")
        assert (got[sl][bound[sl] == 0] == 0).all(), "an element without contributions received a gradient"
    print(f"sorted scatter D={D} F={F} P={P} {cloud}: largest |error| / bound on the binned levels {worst:.3f}")


@pytest.mark.parametrize("lvl_inf", [1, 5])
def test_sorted_scatter_nonfinite_gradient(monkeypatch, lvl_inf):
    """One +inf in dout of a dense (1) or a binned (5) level on the sorted route: that level's gradient holds a non-finite value, the
    other dense levels stay bit-exact and the other binned levels inside their bound."""
    r = hc.scatter_case(3, 8, 2048, "scattered")
    geom = r["geom"]
    g = r["g"].copy()
    g[777, lvl_inf * 2] = np.inf
    got = run_sorted(monkeypatch, r, g, 1.0, padded=True)
    for lvl, binned in enumerate(r["binned"]):
        sl = geom.level_slice(lvl, 2)
        j0 = np.arange(sl.stop - sl.start) % 2 == 0
        if lvl == lvl_inf:
            assert not np.isfinite(got[sl]).all()
            if not binned:
                assert_bits(got[sl][~j0], hc.to_f32_exact(r["ref"][sl][~j0]), "the level's other value")
        elif binned:
            assert (np.abs(got[sl].astype(F64) - r["ref"][sl]) <= r["bound"][sl]).all()
        else:
            assert_bits(got[sl], hc.to_f32_exact(r["ref"][sl]), f"dense level {lvl}")
