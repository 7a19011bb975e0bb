"""Exact tests of the fused field encode (csrc/fused.hip) and its adjoint (csrc/field_bwd.hip) against the float64 reference of
tests/field_cases.py, whose header states what the reference says, derives every bound and lists the routes.  The library is called
through lidar4d_amd._lib with explicit hd_scratch / plane_rows / gd_absmax pointers, on an l4d_field_desc built from
GridMeta(...).desc() and free tensors: the test chooses the route, not the point count.  tests/test_field_cpu.py asserts on the CPU
which kernels every case below reaches.  Run with ``-m gpu`` on an MI355X.

Contracts checked here: gradients are ACCUMULATED (every buffer is prefilled); param_scale multiplies the parameter gradients and
not dflow16; dX = 0 changes nothing and gives dflow16 = 0; slices outside the blended pair keep their bits; rows behind P keep
their bits; element 0 of a scale's static planes turns NaN when a static-plane column of dX holds an inf (nothing else is pinned
about non-finite input)."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_cases as fc
from field_cases import F16, F32, F64, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT16 = F16(-77.0)
RATIOS = {}


def T(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))
    print(f"[field-exact] largest error / bound, {name}: {RATIOS[name]:.3f}")


class DevField:
    """l4d_field_desc of a FieldSpec on the device, as lidar4d_amd.fused._field_desc builds a model's."""

    def __init__(self, spec, table_aligned16=True):
        from lidar4d_amd import ops
        from lidar4d_amd._lib import FieldDesc
        from lidar4d_amd.gridmeta import GridMeta
        self.spec, p = spec, fc.params_of(spec)
        fd = FieldDesc()
        fd.hash_static = GridMeta(*spec.hs.grid_meta_args()).desc()
        buf = torch.zeros(spec.hs.n_entries * 4 + 8, dtype=torch.float16, device=DEV)
        self.hs_table = buf[0 if table_aligned16 else 4:][:spec.hs.n_entries * 4]  # a view offset by 4 halfs is only 8-byte aligned
        self.hs_table.copy_(T(p["hs_table"]))
        assert self.hs_table.data_ptr() % 16 == (0 if table_aligned16 else 8)
        fd.hash_static_table = self.hs_table.data_ptr()
        fd.n_slices = spec.n_slices
        self.hd_tables, self.pairs = [], []
        for pl, g in enumerate(spec.hd):
            fd.hash_dynamic[pl] = GridMeta(*g.grid_meta_args()).desc()
            tabs = [T(t) for t in p["hd_tables"][pl]]
            for s, t in enumerate(tabs):
                fd.hash_dynamic_tables[pl][s] = t.data_ptr()
            pairs = torch.empty(spec.n_slices - 1, g.n_entries, 8, dtype=torch.float16, device=DEV)
            ops.dyn_pairs_build(tabs, pairs)
            fd.hash_dynamic_pairs[pl] = pairs.data_ptr()
            self.hd_tables.append(tabs), self.pairs.append(pairs)
        fd.n_scales, fd.plane_channels = spec.n_scales, spec.C
        for i, v in enumerate([v for r in spec.plane_res for v in r]):
            fd.plane_res[i] = v
        for i, v in enumerate(spec.plane_off):
            fd.plane_off[i] = v
        self.arena = T(fc.to_arena(spec, p["planes"]))
        fd.planes_cl = self.arena.data_ptr()
        self.fd = fd
        assert ops._lib.lib().l4d_field_width(C.byref(fd)) == spec.width


_FIELDS = {}


def field(name, aligned=True):
    if (name, aligned) not in _FIELDS:
        _FIELDS[(name, aligned)] = DevField(fc.SPECS[name], aligned)
    return _FIELDS[(name, aligned)]


def _rows_ws(df):
    from lidar4d_amd import ops
    return torch.empty(ops._lib.lib().l4d_plane_rows_workspace(C.byref(df.fd)) // 4, dtype=torch.float32, device=DEV)


# ---- forward -------------------------------------------------------------------------------------------------------------------------
def run_fwd(df, xt, flow16, tinfo8, in_pad, scratch, rows, sigma_w=None, n_hidden=0):
    from lidar4d_amd import ops
    P = xt.shape[0]
    X = torch.full((P + 3, in_pad), float(SENT16), dtype=torch.float16, device=DEV)
    ws = torch.empty(ops._lib.lib().l4d_density_encode_fwd_workspace(C.byref(df.fd), P) + 16, dtype=torch.uint8, device=DEV) if scratch else None
    rw = _rows_ws(df) if rows else None
    xt_d, fl_d, ti_d = T(xt), T(flow16), T(tinfo8)
    if sigma_w is None:
        ops.call("l4d_density_encode_fwd", C.byref(df.fd), ops._p(xt_d), ops._p(fl_d), ops._p(ti_d), P, ops._p(X), in_pad, ops._p(ws),
                 ops._p(rw), ops._stream())
        torch.cuda.synchronize()
        return X
    y = torch.full((P + 1, 16), float(SENT16), dtype=torch.float16, device=DEV)
    act = torch.empty(n_hidden, P, 64, dtype=torch.float16, device=DEV)
    sigma = torch.empty(P, dtype=torch.float32, device=DEV)
    ops.call("l4d_density_encode_sigma_fwd", C.byref(df.fd), ops._p(xt_d), ops._p(fl_d), ops._p(ti_d), P, ops._p(X), in_pad, ops._p(ws),
             ops._p(rw), ops._p(sigma_w), n_hidden, ops._p(y), ops._p(act), ops._p(sigma), ops._stream())
    torch.cuda.synchronize()
    return X, y, act, sigma


def check_rows(X, c, P, in_pad, what):
    """X [P + 3, in_pad] on the device against the case's rows (row p of a cloud is row p % FULL of the reference)."""
    want, other, near = (T(fc.padded(c[k], in_pad, f)) for k, f in (("want16", F16(1.0)), ("other16", F16(1.0)), ("near", False)))
    idx = torch.arange(P, device=DEV) % fc.FULL
    got = X[:P].view(torch.int16)
    ok = (got == want[idx].view(torch.int16)) | (near[idx] & (got == other[idx].view(torch.int16)))
    bad = torch.nonzero(~ok)
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} of {ok.numel()} elements differ, first (row, column) {bad[:5].tolist()}: got "
                               f"{[float(X[r, k]) for r, k in bad[:5].tolist()]}, want {[float(want[r % fc.FULL, k]) for r, k in bad[:5].tolist()]}")
    assert bool((X[P:] == float(SENT16)).all()), f"{what}: rows behind P were written"
    used = (near[idx] & (got != want[idx].view(torch.int16))).sum().item()
    return used / max(ok.numel(), 1)


@pytest.mark.parametrize("rows", [False, True], ids=["rows-", "rows+"])
@pytest.mark.parametrize("scratch", [False, True], ids=["scratch-", "scratch+"])
def test_forward_rows_every_pointer_combination(scratch, rows):
    """(hd_scratch, plane_rows) in {null, given}^2 at every point count; frames first / middle / last / num_frames = 2 and in_pad
    96 / 128 / 192 in turn; then every frame at 257 points."""
    df = field(8)
    for P, (frame, nf), in_pad in fc.fwd_combo_cases(scratch):
        c = fc.fwd_case(8, frame, nf)
        xt, flow16 = fc.cloud(P, c["t"])
        X = run_fwd(df, xt, flow16, c["tinfo8"], in_pad, scratch, rows)
        check_rows(X, c, P, in_pad, f"encode scratch={scratch} rows={rows} P={P} frame={frame}/{nf} in_pad={in_pad}")


@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "8B"])
def test_forward_both_pair_load_variants(aligned):
    """Static table 16-byte aligned (x-neighbour pair loads, HSMODE 2) and only 8-byte aligned (one load per corner)."""
    df = field(8, aligned)
    for P, (frame, nf) in fc.FWD_PAIR_CASES:
        c = fc.fwd_case(8, frame, nf)
        xt, flow16 = fc.cloud(P, c["t"])
        check_rows(run_fwd(df, xt, flow16, c["tinfo8"], 128, True, True), c, P, 128, f"encode aligned={aligned} P={P}")


@pytest.mark.parametrize("name,in_pad", fc.FWD_OTHER, ids=["L4", "L16", "L6-8"])
def test_forward_other_level_counts(name, in_pad):
    df = field(name)
    c = fc.fwd_case(name, 25, 51)
    for P, scratch, rows in fc.FWD_OTHER_CASES:
        xt, flow16 = fc.cloud(P, c["t"])
        check_rows(run_fwd(df, xt, flow16, c["tinfo8"], in_pad, scratch, rows), c, P, in_pad, f"encode L={name} P={P} {scratch} {rows}")


@pytest.mark.parametrize("name,aligned,points", fc.FWD_BIG_CASES, ids=["levels-in-LDS-kernel", "levels-in-LDS-kernel-8B-table", "levels-launch"])
def test_forward_level_major_route(name, aligned, points):
    """2^18 - 1 points (still gathered), 2^18 and 2^18 + 77 (the static grid level-major: inside the LDS kernel's tasks with equal
    level counts -- with and without the pair loads -- and as a launch of its own otherwise).  The cloud is the 4,161-point cloud repeated."""
    df = field(name, aligned)
    c = fc.fwd_case(name, 25, 51)
    for P in points:
        xt, flow16 = fc.cloud(P, c["t"])
        check_rows(run_fwd(df, xt, flow16, c["tinfo8"], 128, True, True), c, P, 128, f"encode level-major L={name} P={P}")


@pytest.mark.parametrize("n_hidden", [1, 2], ids=["epilogue", "two-launches"])
def test_forward_sigma_entry_point(n_hidden):
    """l4d_density_encode_sigma_fwd at 2^18 + 77 points, in_pad 128: the rows against the reference; y, act, sigma against
    l4d_mlp_fwd_sigma of those rows (tests/test_gpu_mlp_exact.py judges that kernel), bit for bit."""
    from lidar4d_amd import ops
    df = field(8)
    c = fc.fwd_case(8, 22, 51)
    P = fc.FWD_BIG[2]
    xt, flow16 = fc.cloud(P, c["t"])
    r = fc.rng_of(401, n_hidden)
    w = T((r.randn(64 * 128 + 64 * 64 * (n_hidden - 1) + 16 * 64) * 0.05).astype(F16))
    X, y, act, sigma = run_fwd(df, xt, flow16, c["tinfo8"], 128, True, True, sigma_w=w, n_hidden=n_hidden)
    check_rows(X, c, P, 128, f"sigma entry n_hidden={n_hidden}")
    y2, act2, sigma2 = ops.mlp_fwd_sigma(X[:P], w, n_hidden)
    torch.cuda.synchronize()
    assert torch.equal(y[:P].view(torch.int16), y2.view(torch.int16)) and bool((y[P:] == float(SENT16)).all())
    assert torch.equal(act.view(torch.int16), act2.view(torch.int16)) and torch.equal(sigma.view(torch.int32), sigma2.view(torch.int32))


def test_time_setup_is_the_reference_frame_logic():
    from lidar4d_amd import ops
    for nf in (2, 4, 51):
        for frame in range(nf):
            t, ti, ti8 = fc.frame_info(frame, nf)
            got = N(ops.time_setup(torch.tensor([t], dtype=torch.float32, device=DEV), nf))
            assert same_bits(got[:6], ti8[:6]).all(), (nf, frame, got, ti8)


# ---- adjoint -------------------------------------------------------------------------------------------------------------------------
def run_bwd(df, c, rows, use_gd, samples_per_ray, dX=None, zero_prefill=False):
    from lidar4d_amd import ops
    from lidar4d_amd._lib import FieldGrads
    spec, P, in_pad = c["spec"], c["P"], c["in_pad"]
    dX = c["dX"] if dX is None else dX
    z = (lambda a: np.zeros_like(a)) if zero_prefill else (lambda a: a)
    g = dict(arena=T(z(c["g0_arena"])), hs=T(z(c["g0_hs"])), hd=[[T(z(a)) for a in per] for per in c["g0_hd"]])
    fg = FieldGrads()
    fg.hash_static_table, fg.planes_cl = g["hs"].data_ptr(), g["arena"].data_ptr()
    for p in range(3):
        for s in range(spec.n_slices):
            fg.hash_dynamic_tables[p][s] = g["hd"][p][s].data_ptr()
    ws = torch.empty(ops._lib.lib().l4d_density_encode_bwd_workspace(C.byref(df.fd), P) + 16, dtype=torch.uint8, device=DEV)
    dflow = torch.full((P + 2, 16), float(SENT16), dtype=torch.float16, device=DEV)
    rw = _rows_ws(df) if rows else None
    n = spec.colsA // 2
    finite = np.where(np.isfinite(dX[:, n:2 * n].astype(F32)), np.abs(dX[:, n:2 * n].astype(F32)), np.inf)
    vmax = torch.tensor([float(np.abs(fc.to_arena(spec, c["params"]["planes"])).max())], dtype=torch.float32, device=DEV)
    gd = torch.tensor([float(finite.max()) if P else 0.0], dtype=torch.float32, device=DEV) if use_gd else None  # the TRUE maximum
    xt_d, fl_d, ti_d, dX_d = T(c["xt"]), T(c["flow16"]), T(c["tinfo8"]), T(dX)
    ops.call("l4d_density_encode_bwd", C.byref(df.fd), C.byref(fg), ops._p(xt_d), ops._p(fl_d), ops._p(ti_d), P, ops._p(dX_d), in_pad,
             float(c["param_scale"]), ops._p(vmax), int(samples_per_ray), ops._p(ws), ops._p(dflow), ops._p(rw), ops._p(gd), ops._stream())
    torch.cuda.synchronize()
    return dict(arena=N(g["arena"]), hs=N(g["hs"]), hd=[[N(a) for a in per] for per in g["hd"]], dflow=N(dflow))


def assert_bits(got, want, what):
    eq = same_bits(got, want)
    bad = np.flatnonzero(~eq.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {eq.size} differ, first at {bad[:5]}: got {got.reshape(-1)[bad[:5]]}, want {want.reshape(-1)[bad[:5]]}"


def assert_bound(got, ref, bound, what, name):
    err = np.abs(got.astype(F64) - ref)
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (f"{what}: {bad.size} of {err.size} elements beyond their bound, first at {bad[:5]}: got {got.reshape(-1)[bad[:5]]}, "
                           f"want {ref.reshape(-1)[bad[:5]]}, bound {bound.reshape(-1)[bad[:5]]}")
    nz = bound > 0
    if nz.any():
        note(name, (err[nz] / bound[nz]).max())


def check_untouched(c, out, what):
    assert_bits(out["arena"], c["g0_arena"], what + " planes"), assert_bits(out["hs"], c["g0_hs"], what + " static table")
    for p in range(3):
        for s in range(c["spec"].n_slices):
            assert_bits(out["hd"][p][s], c["g0_hd"][p][s], f"{what} slice table {p}.{s}")


def check_dflow(c, out, what):
    P = c["P"]
    d = out["dflow"]
    assert (d[P:] == SENT16).all(), f"{what}: dflow16 rows behind P were written"
    assert_bits(d[:P, 6:], np.zeros((P, 10), F16), what + " dflow16 columns 6 .. 15")
    assert_bound(d[:P, :6], c["dflow"], c["dflow_bound"], what + " dflow16", "dflow16")
    if not c["tinfo"][3]:
        assert_bits(d[:P, :3], np.zeros((P, 3), F16), what + " dflow16 forward (last frame)")
    if not c["tinfo"][4]:
        assert_bits(d[:P, 3:6], np.zeros((P, 3), F16), what + " dflow16 backward (first frame)")


def check_bwd(c, out, what):
    spec = c["spec"]
    if c["P"] == 0:
        return check_untouched(c, out, what)
    for s in range(spec.n_scales):
        for ci in range(6):
            sl = spec.plane_slice(s, ci)
            assert_bound(out["arena"][sl], c["arena"][sl], c["bound"][sl], f"{what} plane {s}.{ci}", "static planes" if ci in fc.pw.STATIC else "time planes")
    assert_bits(out["hs"], c["hs_bits"], what + " static table")
    for p in range(3):
        for s in range(spec.n_slices):
            assert_bits(out["hd"][p][s], c["hd_bits"][p][s], f"{what} slice table {p}.{s}")
    check_dflow(c, out, what)


@pytest.mark.parametrize("name,in_pad", fc.BWD_PREP, ids=["L4-unstaged-prep", "L8-fused-prep", "L16-wide"])
def test_adjoint_every_point_count(name, in_pad):
    """plane_rows and gd_absmax given, samples_per_ray = 0: the un-staged prep kernel (12 dynamic columns), the time-plane kernel
    with the preparation pass inside (24), the wide one (48); one and two chunks with a ragged last one."""
    df = field(name)
    for i, P in enumerate(fc.BWD_POINTS):
        (frame, nf), ps = fc.bwd_args(i)
        c = fc.bwd_case(name, P, frame, nf, in_pad, ps)
        check_bwd(c, run_bwd(df, c, True, True, 0), f"adjoint L={name} P={P} frame={frame}/{nf} param_scale={ps}")


@pytest.mark.parametrize("rows,use_gd", fc.BWD_OTHER_POINTERS, ids=["rows- gd-", "rows+ gd-", "rows- gd+"])
@pytest.mark.parametrize("name,in_pad", fc.BWD_PREP, ids=["L4", "L8", "L16"])
def test_adjoint_other_pointer_combinations(name, in_pad, rows, use_gd):
    """The prep kernel (staged for 24 / 48 dynamic columns) in front of planes_dyn_lds_kernel<false, false> / <true, false>."""
    df = field(name)
    for i, P in enumerate(fc.BWD_OTHER_POINTS):
        (frame, nf), ps = fc.bwd_args(i + 1)
        c = fc.bwd_case(name, P, frame, nf, in_pad, ps)
        check_bwd(c, run_bwd(df, c, rows, use_gd, 0), f"adjoint L={name} P={P} rows={rows} gd={use_gd} frame={frame}/{nf}")


def test_adjoint_range_tasks():
    """xy stack of 2^16 entries: a dense level of 36,864 entries walked as three ranges, a hashed one as four."""
    df = field("6/8")
    for P, (frame, nf) in fc.BWD_RANGE_CASES:
        c = fc.bwd_case("6/8", P, frame, nf, 96, 1.0)
        check_bwd(c, run_bwd(df, c, True, True, 0), f"adjoint range tasks P={P}")


@pytest.mark.parametrize("n_rays", fc.BAND_RAYS)
def test_adjoint_band_skip(n_rays):
    """samples_per_ray = 64 on a cloud of rays: the wave-level band skip of planes_static_lds_kernel, whole-segment chunks."""
    df = field(8)
    c = fc.band_case(n_rays)
    out = run_bwd(df, c, True, True, 64)
    what = f"adjoint band skip {n_rays} rays"
    spec = c["spec"]
    for s in range(spec.n_scales):
        for ci in range(6):
            sl = spec.plane_slice(s, ci)
            assert_bound(out["arena"][sl], c["arena"][sl], c["bound"][sl], f"{what} plane {s}.{ci}", "static planes (rays)" if ci in fc.pw.STATIC else "time planes (rays)")
    assert_bits(out["hs"], c["g0_hs"], what + " static table (no gradient)")
    for p in range(3):
        for s in range(spec.n_slices):
            ref, bound = c["hd_ref"][p][s]
            if not bound.any():
                assert_bits(out["hd"][p][s], c["g0_hd"][p][s], f"{what} slice table {p}.{s} (outside the pair)")
            else:
                assert_bound(out["hd"][p][s], ref, bound, f"{what} slice table {p}.{s}", "slice tables (rays)")
    check_dflow(c, out, what)


def test_adjoint_of_a_zero_gradient_changes_nothing():
    df = field(8)
    for rows, use_gd in ((True, True), (False, False)):
        c = dict(fc.bwd_case(8, 1025, 25, 51, 128, 1.0))
        dX = c["dX"].copy()
        dX[:, :c["spec"].width] = 0.0
        out = run_bwd(df, c, rows, use_gd, 0, dX=dX)
        check_untouched(c, out, "dX = 0")
        assert_bits(out["dflow"][:1025], np.zeros((1025, 16), F16), "dX = 0: dflow16")


def test_param_scale_multiplies_parameter_gradients_only():
    """Same inputs at param_scale 1 and 2^-7 on zeroed buffers: dflow16 keeps its bits, the hash gradients scale exactly."""
    df = field(8)
    a = fc.bwd_case(8, 1025, 25, 51, 128, 1.0)
    b = fc.bwd_case(8, 1025, 25, 51, 128, 2.0 ** -7)
    oa, ob = run_bwd(df, a, True, True, 0, zero_prefill=True), run_bwd(df, b, True, True, 0, zero_prefill=True)
    assert_bits(oa["dflow"], ob["dflow"], "dflow16 under param_scale")
    assert oa["dflow"][:1025, :6].any()
    assert_bits((oa["hs"].astype(F64) * 2.0 ** -7).astype(F32), ob["hs"], "static table under param_scale")


def test_nonfinite_upstream_gradient_reaches_the_planes():
    """One inf in a static-plane column of scale 1: element 0 of that scale's static planes turns NaN (planes_static_lds_kernel)."""
    df = field(8)
    c = dict(fc.bwd_case(8, 1025, 25, 51, 128, 1.0))
    dX = c["dX"].copy()
    dX[300, 8 + 3] = np.inf
    out = run_bwd(df, c, True, True, 0, dX=dX)
    for ci in fc.pw.STATIC:
        assert np.isnan(out["arena"][c["spec"].plane_off[1 * 6 + ci]]), ci
