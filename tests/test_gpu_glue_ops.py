"""Operator-level tests of the small kernels between the fused operators, on the device (``-m gpu``, MI355X), each against a
reference that no HIP code computed (tests/glue_cases.py): the scene-flow glue of csrc/glue.hip, the chamfer distance at its
edges, the attribute and density-activation glue of csrc/render.hip, and the hex-plane sampler with unequal resolutions.

Every test names its kind of reference: E (exact emulation in numpy fp32 / fp16, bit-equal), L (lattice inputs, bit-equal to
float64 in any summation order) or X (expf inside: fp16(float64), either neighbour within EXP_ULPS fp32 ulps of a rounding
midpoint).  The rules, the cases and why they are these: tests/glue_cases.py; the references themselves: tests/test_glue_cpu.py."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import glue_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32, F64 = np.float16, np.float32, np.float64
SENT = F32(-12345.0)


def _ops():
    from lidar4d_amd import ops
    return ops


def _err():
    from lidar4d_amd._lib import HipExtensionError
    return HipExtensionError


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, float(value), dtype=dtype, device=DEV)


def assert_bits(got, want, what):
    got = host(got) if torch.is_tensor(got) else got
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(~gc.same_bits(got, want).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[:6]}: got {got.reshape(-1)[bad[:6]]}, want {want.reshape(-1)[bad[:6]]}"


def _default_bound():
    from lidar4d_amd.lidar4d import LiDAR4D
    return float(inspect.signature(LiDAR4D.__init__).parameters["bound"].default)


# =================================================================================================================================
# 1. scene-flow glue
# =================================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_flow_xt(n):
    """E.  bound 1.0, the model's default, and 1.5 (a divisor that is no power of two, so the division rounds)."""
    ops = _ops()
    for bound in sorted({1.0, _default_bound(), 1.5}):
        pc = gc.rng_of(1, n).uniform(-2 * bound, 2 * bound, size=(n, 3)).astype(F32)
        if n >= 255:
            pc[0], pc[1], pc[2] = bound, -bound, 0.0
            assert (np.abs(pc) > bound).any() and (np.abs(pc) < bound).any()
        t = np.array([0.3701171], F32)
        xt = ops.flow_xt(dev(pc), dev(t), bound)
        assert_bits(xt, gc.flow_xt_ref(pc, t[0], bound), f"flow_xt n={n} bound={bound}")
        assert_bits(xt[:, 3], np.full(n, t[0], F32), "flow_xt: column 3 carries t")


FLOW_WARPS = [[(0, 0.25)], [(3, -0.25), (0, 0.5)], [(0, -0.5), (3, 1.0 / 50), (0, -1.0 / 50)],
              [(0, 0.25), (3, -0.25), (0, 0.5), (3, -0.5)], [(3, -1.0 / 50), (0, 1.0 / 50), (3, 0.25), (0, -0.5)]]


@pytest.mark.parametrize("n", [1, 257])
def test_flow_warp(n):
    """E: product rounded, then sum rounded.  Columns 6..15 of y16 hold NaN and must not reach the output."""
    ops = _ops()
    r = gc.rng_of(2, n)
    pc = r.uniform(-1, 1, size=(n, 3)).astype(F32)
    y16 = np.full((n, 16), np.nan, F16)
    y16[:, :6] = r.uniform(-0.3, 0.3, size=(n, 6)).astype(F16)
    for variants in FLOW_WARPS:
        out = ops.flow_warp(dev(pc), dev(y16), variants)
        assert out.shape == (len(variants), n, 3)
        assert_bits(out, gc.flow_warp_ref(pc, y16, variants), f"flow_warp n={n} {variants}")
        assert bool(torch.isfinite(out).all())


def test_flow_warp_rejects_bad_arguments():
    ops = _ops()
    pc, y16 = filled((4, 3), 0.5), filled((4, 16), 0.25, torch.float16)
    out = filled((5, 4, 3), SENT)
    col0, step = (C.c_int32 * 5)(0, 3, 0, 3, 0), (C.c_float * 5)(1, 1, 2, 2, 1)
    with pytest.raises(_err()):
        ops.call("l4d_flow_warp", ops._p(pc), ops._p(y16), 4, 5, col0, C.cast(step, C.c_void_p), ops._p(out), ops._stream())
    with pytest.raises(_err()):
        ops.flow_warp(pc, y16, [(6, 0.25)])
    with pytest.raises(_err()):
        ops.flow_warp(pc, y16, [(0, 0.25), (-1, 0.25)])
    assert_bits(out, np.full((5, 4, 3), SENT, F32), "flow_warp: refused calls write nothing")


@pytest.mark.parametrize("n,m,same", [(n, m, False) for n, m in gc.FLOW_GRAD_SHAPES] + [(300, 299, True)])
def test_flow_chamfer_grad(n, m, same):
    """L.  dist / idx from the numpy brute force; three terms in the forward + 1 / forward + 2 / backward pattern on prefilled dy;
    ``same``: every q is nearest to p[0], 299 atomics on one row."""
    ops = _ops()
    c = gc.flow_grad_case(n, m, same_neighbour=same)
    dy, ref = dev(c["dy0"]), c["dy0"].astype(F64)
    blocks = (max(n, m) + 255) // 256
    for v, t in enumerate(c["terms"]):
        partial = filled((blocks + 3,), SENT)
        args = [dev(t[k]) for k in ("p", "q", "dist1", "dist2", "idx1", "idx2")]
        ops.call("l4d_flow_chamfer_grad", ops._p(args[0]), n, ops._p(args[1]), m, ops._p(args[2]), ops._p(args[3]), ops._p(args[4]),
                 ops._p(args[5]), float(t["step"]), int(t["col0"]), ops._p(dy), ops._p(partial), ops._stream())
        want = gc.flow_chamfer_grad_ref(t, ref)
        assert want.shape == (blocks,)
        assert_bits(partial, np.concatenate([gc.to_f32_exact(want), np.full(3, SENT, F32)]), f"partial of term {v}")
        assert_bits(dy, gc.to_f32_exact(ref), f"dy after term {v} (columns outside col0..col0+2 untouched)")


def test_flow_chamfer_grad_rejects_other_columns():
    ops = _ops()
    t = gc.flow_grad_case(1, 1)["terms"][0]
    args = [dev(t[k]) for k in ("p", "q", "dist1", "dist2", "idx1", "idx2")]
    dy, partial = filled((1, 6), SENT), filled((2,), SENT)
    for col0 in (1, 2, 4, 6, -1):
        with pytest.raises(_err()):
            ops.call("l4d_flow_chamfer_grad", ops._p(args[0]), 1, ops._p(args[1]), 1, ops._p(args[2]), ops._p(args[3]), ops._p(args[4]),
                     ops._p(args[5]), 0.25, col0, ops._p(dy), ops._p(partial), ops._stream())
    assert_bits(dy, np.full((1, 6), SENT, F32), "refused calls write nothing")


def _finish(c, w):
    ops = _ops()
    ng = 0 if c["y_g"] is None else c["y_g"].shape[0]
    partial, dy = dev(c["partial"]), dev(c["dy"])
    y_g = None if ng == 0 else dev(c["y_g"])
    dy_g = None if ng == 0 else filled((ng + 1, 6), SENT)
    loss, amax = filled((2,), SENT), filled((3,), SENT)
    ops.call("l4d_flow_loss_finish", ops._p(partial), int(c["partial"].size), ops._p(y_g), ng, float(w), ops._p(dy_g), ops._p(dy),
             int(c["dy"].size), ops._p(loss), ops._p(amax), ops._stream())
    return host(loss), None if dy_g is None else host(dy_g), host(amax)


@pytest.mark.parametrize("ng", gc.FINISH_GROUND)
@pytest.mark.parametrize("n_partial", gc.FINISH_PARTIALS)
def test_flow_loss_finish(n_partial, ng):
    """L: integer partials, ground flows on 2^-8, w_ground = 2^-10; n_dy even and odd (the tail branch)."""
    for n_dy in (6 * 211, 6 * 211 + 1, 1, 0):
        c = gc.finish_case(n_partial, ng, n_dy)
        want_loss, want_dyg, want_amax, _ = gc.flow_loss_finish_ref(c, gc.W_GROUND_LATTICE)
        loss, dy_g, amax = _finish(c, gc.W_GROUND_LATTICE)
        assert_bits(loss, np.array([F32(want_loss), SENT], F32), f"loss n_dy={n_dy}")
        assert_bits(amax, np.array([want_amax[0], want_amax[1], SENT], F32), f"amax n_dy={n_dy}")
        if ng:
            assert_bits(dy_g, np.concatenate([want_dyg, np.full((1, 6), SENT, F32)]), "dy_g = w * sign, +0 at +-0")


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_flow_loss_finish_amax_is_inf_for_nonfinite_dy(bad):
    for n_dy, pos in ((1266, 0), (1266, 1265), (1267, 1266), (1267, 0), (1267, 700), (1, 0)):
        c = gc.finish_case(5, 3, n_dy)
        c["dy"][pos] = bad
        _, _, amax = _finish(c, gc.W_GROUND_LATTICE)
        assert amax[0] == np.inf and amax[1] == F32(gc.W_GROUND_LATTICE), (n_dy, pos, amax)


def test_flow_loss_finish_real_weight():
    """w_ground = 0.001 and real-valued terms: |loss - float64| <= len * 2^-24 * sum |terms|, which holds for any summation order."""
    c = gc.finish_case(3000, 1500, 600, lattice=False)
    want, want_dyg, want_amax, bound = gc.flow_loss_finish_ref(c, 0.001, lattice=False)
    loss, dy_g, amax = _finish(c, 0.001)
    print(f"flow_loss_finish, w = 0.001: loss {loss[0]:.9g}, float64 {want:.12g}, |diff| {abs(float(loss[0]) - want):.3e}, bound {bound:.3e}")
    assert abs(float(loss[0]) - want) <= bound and bound < 1e-2 * want
    assert_bits(dy_g[:-1], want_dyg, "dy_g")
    assert_bits(amax[:2], want_amax, "amax")


@pytest.mark.parametrize("n", [1, 256, 257])
def test_flow_dy16(n):
    """k is read back from inv_out (an exact power of two) and judged in float64; given k, the six columns are E."""
    ops = _ops()
    r = gc.rng_of(3, n)
    unit = r.uniform(-1, 1, size=(n, 6)).astype(F32)
    unit[0, 0], unit[-1, 5] = 1.0, 0.0
    for amax, g, kind in gc.dy16_scales():
        dy = unit * amax
        dy16, inv = filled((n + 1, 16), 7.0, torch.float16), filled((2,), SENT)
        keep = (dev(dy), dev([g], F32), dev([amax], F32))  # (alive until the launch: a freed block is handed to the next allocation)
        ops.call("l4d_flow_dy16", ops._p(keep[0]), n, ops._p(keep[1]), ops._p(keep[2]), ops._p(dy16), ops._p(inv), ops._stream())
        inv = host(inv)
        mant, e = np.frexp(F64(inv[0]))
        assert mant == 0.5 and inv[1] == SENT, f"inv_out {inv[0]!r} is no power of two"
        k = -(int(e) - 1)
        a = F64(amax) * abs(F64(g))
        what = f"amax={amax!r} g={g!r} ({kind}): k={k}"
        if kind == "clamp+":
            assert k == 40, what
        elif kind == "clamp-":
            assert k == -40, what
        else:
            # [2^11, 2^12), widened by 2 fp32 ulps at either end: within 2 ulps of a power of two either neighbouring k is accepted
            assert -40 < k < 40 and 2048.0 * (1 - 2 * 2.0 ** -24) <= a * 2.0 ** k < 4096.0 * (1 + 2 * 2.0 ** -23), what
            if kind == "k":
                assert 2048.0 <= a * 2.0 ** k < 4096.0, what
        want = np.concatenate([gc.dy16_ref(dy, g, k), np.full((1, 16), 7.0, F16)])
        assert_bits(dy16, want, what)


@pytest.mark.parametrize("amax,g", [(np.inf, 1.0), (np.nan, 1.0), (np.inf, -0.5), (1.0, np.inf), (1.0, -np.inf), (1.0, np.nan), (np.inf, np.nan)])
def test_flow_dy16_hands_nonfinite_scales_on(amax, g):
    """common.h f2h_grad: a non-finite upstream gradient or amax makes every one of the six columns of every row non-finite."""
    ops = _ops()
    n = 257
    dy = gc.rng_of(4).uniform(-1, 1, size=(n, 6)).astype(F32)
    dy[0], dy[5, 2] = 0.0, 1e-20
    dy16, inv = filled((n, 16), 7.0, torch.float16), filled((1,), SENT)
    keep = (dev(dy), dev([g], F32), dev([amax], F32))
    ops.call("l4d_flow_dy16", ops._p(keep[0]), n, ops._p(keep[1]), ops._p(keep[2]), ops._p(dy16), ops._p(inv), ops._stream())
    out = host(dy16)
    assert not np.isfinite(out[:, :6]).any(), f"{int(np.isfinite(out[:, :6]).sum())} finite values of {6 * n}"
    assert_bits(out[:, 6:], np.zeros((n, 10), F16), "columns 6..15")


@pytest.mark.parametrize("n", gc.AXPY_SIZES)
def test_axpy_dev(n):
    """E: y += fp32(a * x) where x != 0; where x == 0, y keeps its bits (NaN and -0.0 included)."""
    ops = _ops()
    y, x, a = gc.axpy_case(n)
    yd = dev(np.concatenate([y, np.array([SENT, SENT], F32)]))
    xd = dev(np.concatenate([x, np.array([1.0, 1.0], F32)]))
    ad = dev([a], F32)
    ops.call("l4d_axpy_dev", ops._p(yd), ops._p(xd), n, ops._p(ad), ops._stream())
    assert_bits(yd, np.concatenate([gc.axpy_ref(y, x, a), np.array([SENT, SENT], F32)]), f"axpy n={n}")


@pytest.mark.parametrize("na,nb", [(n, 7) for n in gc.AXPY_SIZES] + [(7, n) for n in gc.AXPY_SIZES[:-1]] + [(0, 0), (300, 0), (0, 300), (256, 256)])
def test_scale_buffers(na, nb):
    """E: out = in * s[0] for two buffers in one launch; na = 0 and nb = 0 each on its own."""
    ops = _ops()
    r = gc.rng_of(6, na, nb)
    a, b = r.uniform(-3, 3, size=na).astype(F32), r.uniform(-3, 3, size=nb).astype(F32)
    s = F32(r.uniform(0.1, 1000.0))
    oa, ob = filled((na + 2,), SENT), filled((nb + 2,), SENT)
    ad, bd = dev(a), dev(b)
    sd = dev([s], F32)
    ops.call("l4d_scale_buffers", ops._p(ad), ops._p(oa), na, ops._p(bd), ops._p(ob), nb, ops._p(sd), ops._stream())
    tail = np.array([SENT, SENT], F32)
    assert_bits(oa, np.concatenate([a * s, tail]), "out_a")
    assert_bits(ob, np.concatenate([b * s, tail]), "out_b")


# =================================================================================================================================
# 2. chamfer edges
# =================================================================================================================================
def _chamfer_fwd(xyz1, xyz2, b=None, n=None, m=None):
    ops = _ops()
    b = xyz1.shape[0] if b is None else b
    n = xyz1.shape[1] if n is None else n
    m = xyz2.shape[1] if m is None else m
    d1, d2 = filled((max(b, 1), max(n, 1)), SENT), filled((max(b, 1), max(m, 1)), SENT)
    i1 = torch.full((max(b, 1), max(n, 1)), -7, dtype=torch.int32, device=DEV)
    i2 = torch.full((max(b, 1), max(m, 1)), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(ops._lib.lib().l4d_chamfer_workspace(b, n, m)), 8), dtype=torch.uint8, device=DEV)
    a1, a2 = dev(xyz1), dev(xyz2)
    ops.call("l4d_chamfer_fwd", ops._p(a1), ops._p(a2), b, n, m, ops._p(d1), ops._p(d2), ops._p(i1), ops._p(i2), ops._p(ws), ops._stream())
    return host(d1), host(d2), host(i1), host(i2)


def _check_chamfer(xyz1, xyz2, what):
    want = gc.chamfer_ref(xyz1, xyz2)
    got = _chamfer_fwd(xyz1, xyz2)
    for g, w, name in zip(got, want, ("dist1", "dist2", "idx1", "idx2")):
        if name.startswith("idx"):
            assert np.array_equal(g, w), f"{what} {name}: {int((g != w).sum())} differ, first at {np.argwhere(g != w)[:4].tolist()}"
        else:
            assert_bits(g, w, f"{what} {name}")
    n, m = xyz1.shape[1], xyz2.shape[1]
    assert got[2].min() >= 0 and got[2].max() < m and got[3].min() >= 0 and got[3].max() < n
    return got


@pytest.mark.parametrize("b,n,m", gc.CHAMFER_SHAPES)
def test_chamfer_edges(b, n, m):
    """Brute force in numpy fp32 with the kernel's expression order, strict <, first minimum: dist and idx bit-equal.  Lattice
    clouds (natural ties), exact copies of one candidate in two segments and twice in one tile, a query equal to a candidate."""
    segs, seg_len = gc.seg_for(n, m, b)
    if (b, n, m) in gc.CHAMFER_MULTI_SEGMENT:
        assert segs > 1
    if (b, n, m) == (1, 300, 3000):
        assert (segs, seg_len) == (3, 1000) and seg_len % 1024 != 0
    xyz1, xyz2 = gc.chamfer_case(b, n, m)
    d1, d2, i1, i2 = _check_chamfer(xyz1, xyz2, f"chamfer {b}x{n}x{m}")
    J = gc.plant_indices(m)
    if J:
        assert (d1[:, 0] == 0.0).all() and (i1[:, 0] == J[0]).all()
    if gc.plant_indices(n):
        assert (d2[:, 0] == 0.0).all() and (i2[:, 0] == gc.plant_indices(n)[0]).all()


def test_chamfer_nonfinite_coordinates_keep_indices_in_range():
    """A query with a NaN or an inf coordinate: every index in [0, m), dist what the brute force gives with the same strict < and
    the same 3.4e38 start (the contract in the header comment of l4d_chamfer_fwd; the backward indexes with these)."""
    xyz1, xyz2 = gc.chamfer_case(1, 300, 3000)
    xyz1[0, 5], xyz1[0, 6], xyz1[0, 299] = (np.nan, 0.1, 0.2), (np.inf, 0.0, 0.0), (0.0, -np.inf, np.nan)
    xyz2[0, 100], xyz2[0, 2999], xyz2[0, 1000] = (0.0, np.nan, 0.0), (-np.inf, 0.0, 0.0), (np.nan, np.nan, np.nan)
    d1, d2, i1, i2 = _check_chamfer(xyz1, xyz2, "chamfer with nan / inf")
    for q in (5, 6, 299):
        assert d1[0, q] == gc.CHAMFER_START and i1[0, q] == 0
    for q in (100, 2999, 1000):
        assert d2[0, q] == gc.CHAMFER_START and i2[0, q] == 0
    assert not np.isin(i1[0], (100, 2999, 1000)).any() and not np.isin(i2[0], (5, 6, 299)).any()


def test_chamfer_empty_clouds():
    ops = _ops()
    one = np.zeros((1, 1, 3), F32)
    five = np.zeros((1, 5, 3), F32)
    with pytest.raises(_err()):
        _chamfer_fwd(one[:, :0], five)
    with pytest.raises(_err()):
        _chamfer_fwd(five, one[:, :0])
    for b, n, m in ((1, 0, 0), (0, 4, 5), (0, 0, 0)):
        d1, d2, i1, i2 = _chamfer_fwd(five, five, b=b, n=n, m=m)
        assert (d1 == SENT).all() and (d2 == SENT).all() and (i1 == -7).all() and (i2 == -7).all()
    g = filled((1, 5, 3), SENT)
    a, idx, gd = dev(five), torch.zeros(1, 5, dtype=torch.int32, device=DEV), filled((1, 5), 1.0)
    for b, n, m in ((0, 5, 5), (1, 0, 5), (1, 5, 0)):
        ops.call("l4d_chamfer_bwd", ops._p(a), ops._p(a), b, n, m, ops._p(gd), ops._p(gd), ops._p(idx), ops._p(idx), ops._p(g), ops._p(g), ops._stream())
    assert (host(g) == SENT).all()


@pytest.mark.parametrize("b,n,m", [(1, 300, 3), (1, 3, 300), (2, 257, 255)])
def test_chamfer_bwd_lattice(b, n, m):
    """L: both gradients bit-equal to float64, on top of a prefill; with 3 candidates a hundred queries share one neighbour."""
    ops = _ops()
    xyz1 = np.stack([gc.lattice_cloud(n, 4, (n, m, 1, i)) for i in range(b)])
    xyz2 = np.stack([gc.lattice_cloud(m, 4, (n, m, 2, i)) for i in range(b)])
    _, _, i1, i2 = gc.chamfer_ref(xyz1, xyz2)
    gd1 = (gc.rng_of(43, n).randint(-8, 9, size=(b, n)) / 4.0).astype(F32)
    gd2 = (gc.rng_of(47, m).randint(-8, 9, size=(b, m)) / 4.0).astype(F32)
    g1_0, g2_0 = np.full((b, n, 3), 0.25, F32), np.full((b, m, 3), -0.5, F32)
    want1, want2 = gc.chamfer_bwd_ref(xyz1, xyz2, gd1, gd2, i1, i2, g1_0, g2_0)
    g1, g2 = dev(g1_0), dev(g2_0)
    t = [dev(v) for v in (xyz1, xyz2, gd1, gd2, i1, i2)]
    ops.call("l4d_chamfer_bwd", ops._p(t[0]), ops._p(t[1]), b, n, m, ops._p(t[2]), ops._p(t[3]), ops._p(t[4]), ops._p(t[5]), ops._p(g1),
             ops._p(g2), ops._stream())
    assert_bits(g1, gc.to_f32_exact(want1), "grad_xyz1")
    assert_bits(g2, gc.to_f32_exact(want2), "grad_xyz2")
    if min(n, m) == 3:
        assert np.bincount((i1 if n > m else i2)[0], minlength=3).max() >= 100


# =================================================================================================================================
# 3. attribute and density-activation glue
# =================================================================================================================================
@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("n_enc,n_geo,in_pad", gc.GATHER_WIDTHS)
def test_attr_gather(n_enc, n_geo, in_pad, with_idx):
    """Bit-exact copy: [direction encoding | geo features = h[:, 1 : 1 + n_geo] | 1.0 ...], rows >= min(count, cap) untouched."""
    ops = _ops()
    for cap, T in ((1, 1), (255, 7), (257, 64), (257, 1), (1, 64)):
        c = gc.gather_case(n_enc, n_geo, in_pad, cap, T, with_idx)
        d_enc, h = dev(c["dir_enc"]), dev(c["h"])
        idx = None if c["idx"] is None else dev(c["idx"])
        for count in (None, 0, cap // 2, cap, cap + 5):
            xa = filled((cap, in_pad), gc.SENTINEL16, torch.float16)
            cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
            out = ops.attr_gather(idx, cnt, cap, T, d_enc, h, n_geo, in_pad, xa=xa)
            assert out is xa
            got = host(xa)
            assert_bits(got, gc.attr_gather_ref(c, count), f"attr_gather cap={cap} T={T} count={count}")
            assert not np.isnan(got).any()  # column 0 of h is NaN
            M = cap if count is None else min(count, cap)
            assert (got[:M, n_enc + n_geo:] == 1.0).all() and (got[M:] == gc.SENTINEL16).all()


def test_attr_gather_rejects_bad_widths():
    ops = _ops()
    h, d = filled((8, 16), 1.0, torch.float16), filled((8, 16), 1.0, torch.float16)
    for n_geo, in_pad in ((3, 20), (16, 32), (15, 24)):  # in_pad % 8, n_geo > 15, n_enc + n_geo > in_pad
        xa = filled((8, 96), gc.SENTINEL16, torch.float16)
        with pytest.raises(_err()):
            ops.attr_gather(None, None, 8, 1, d, h, n_geo, in_pad, xa=xa)
        assert (host(xa) == gc.SENTINEL16).all()


def test_attr_scatter_every_fp16_input():
    """X, exhaustive: one row per fp16 bit pattern in either channel (in opposite orders)."""
    ops = _ops()
    x = gc.all_f16()
    cap, P = 65536, 65536 + 100
    y_r, y_i = np.full((cap, 16), np.nan, F16), np.full((cap, 16), np.nan, F16)
    y_r[:, 0], y_i[:, 0] = x, x[::-1]
    idx = gc.work_list(P, cap, (9,))
    dense, compact = filled((P, 2), SENT), filled((cap, 2), SENT)
    ops.attr_scatter(dev(idx), None, cap, dev(y_r), dev(y_i), dense, compact)
    dense, compact = host(dense), host(compact)
    assert_bits(dense[idx], compact, "attr_dense[idx[j]] == attr_compact[j]")
    rest = np.ones(P, bool)
    rest[idx] = False
    assert rest.sum() == 100 and (dense[rest] == SENT).all()
    for ch, xin in ((0, x), (1, x[::-1])):
        got = compact[:, ch]
        got16 = got.astype(F16)
        assert_bits(got16.astype(F32), got, "the outputs are fp16 values")
        fin = np.isfinite(xin)
        n_near, worst = gc.x_check(got16[fin], gc.sigmoid64(xin[fin]), f"sigmoid channel {ch}")
        print(f"l4d_attr_scatter channel {ch}: {n_near} near-boundary cases, largest distance among differing cases {worst:.2f} fp32 ulps")
        assert np.isnan(got[np.isnan(xin)]).all() and got[xin == np.inf][0] == 1.0 and got[xin == -np.inf][0] == 0.0
        assert (got[xin == 0] == 0.5).all() and (xin == 0).sum() == 2
        ok = ~np.isnan(xin)
        order = np.argsort(xin[ok].astype(F64), kind="stable")
        assert (np.diff(got[ok][order]) >= 0).all(), "not monotone"
        assert got[ok].min() >= 0.0 and got[ok].max() <= 1.0
    # either output may be absent; a count below cap leaves the other rows alone
    n = 300
    cnt = torch.tensor([n - 3], dtype=torch.int32, device=DEV)
    for use_dense, use_compact in ((True, False), (False, True)):
        d2, c2 = filled((P, 2), SENT), filled((n, 2), SENT)
        ops.attr_scatter(dev(idx[:n]), cnt, n, dev(y_r[20000:20000 + n]), dev(y_i[20000:20000 + n]), d2 if use_dense else None,
                         c2 if use_compact else None)
        d2, c2 = host(d2), host(c2)
        want = compact[20000:20000 + n - 3]  # the same input rows as in the exhaustive launch
        if use_dense:
            assert_bits(d2[idx[:n - 3]], want, "dense only")
            assert (d2[idx[n - 3:n]] == SENT).all() and (c2 == SENT).all()
        else:
            assert_bits(c2[:n - 3], want, "compact only")
            assert (c2[n - 3:] == SENT).all() and (d2 == SENT).all()


def test_attr_scatter_bwd():
    """E: fp16(((d * s) * (1 - s)) * loss_scale) in column 0, +0 in columns 1..15; nothing saturates."""
    ops = _ops()
    r = gc.rng_of(8)
    s_edge = np.array([0.0, 2.0 ** -11, 0.25, 0.5, 1.0 - 2.0 ** -11, 1.0], F32)
    d_edge = np.array([1.0, -3.5, 1e-3, np.inf, -np.inf, np.nan, 3e4, -6e5, 0.0, 2100.0], F32)
    s = np.concatenate([np.repeat(s_edge, d_edge.size), gc.sigmoid64(r.uniform(-8, 8, size=400)).astype(F16).astype(F32)])
    d = np.concatenate([np.tile(d_edge, s_edge.size), (r.standard_normal(400) * 50).astype(F32)])
    cap, P = s.size, s.size + 33
    idx = gc.work_list(P, cap, (10,))
    compact = np.stack([s, s[::-1]], -1).astype(F32)
    d_attr = np.full((P, 2), np.nan, F32)
    d_attr[idx, 0], d_attr[idx, 1] = d, np.roll(d, 7)
    for loss_scale in (128.0, 1.0):
        dy_r, dy_i = filled((cap, 16), np.nan, torch.float16), filled((cap, 16), np.nan, torch.float16)
        ops.attr_scatter_bwd(dev(idx), None, cap, dev(d_attr), dev(compact), loss_scale, dy_r, dy_i)
        want_r, want_i = gc.attr_scatter_bwd_ref(d_attr, compact, idx, loss_scale)
        assert_bits(dy_r, want_r, "dy_raydrop")
        assert_bits(dy_i, want_i, "dy_intensity")
        if loss_scale == 128.0:
            col = want_r[:, 0]
            assert np.isinf(col[np.isfinite(d)]).any() and np.isnan(col).any() and not (np.abs(col) == 65504.0).any()


@pytest.mark.parametrize("in_pad,n_enc,n_geo,h_layout,rows", [c + (True,) for c in gc.GATHER_BWD_ROWS] + [c + (False,) for c in gc.GATHER_BWD_GENERIC])
def test_attr_gather_bwd(in_pad, n_enc, n_geo, h_layout, rows):
    """E: fp32 sum of two fp16, then fp16.  The row kernel writes the whole row (column 0 and columns above n_geo +0); the generic
    kernel leaves them untouched (sentinel).  60000 + 60000 = inf, inf - inf = NaN."""
    ops = _ops()
    cap, P = 257, 300
    c = gc.gather_bwd_case(in_pad, n_enc, n_geo, cap, P)
    for count in (None, 100):
        dh = filled((P, 16), gc.SENTINEL16, torch.float16)
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
        ops.attr_gather_bwd(dev(c["idx"]), cnt, cap, dev(c["dxa_r"]), dev(c["dxa_i"]), in_pad, n_enc, n_geo, dh, h_layout=bool(h_layout))
        want = gc.attr_gather_bwd_ref(c, in_pad, n_enc, n_geo, h_layout, rows, count)
        assert_bits(dh, want, f"attr_gather_bwd count={count}")
    row0 = want[c["idx"][0]]
    assert np.isinf(row0).any() and np.isnan(row0).any()
    if rows:
        assert (want[c["idx"][:100], 0] == 0).all() and (want[c["idx"][:100], 1 + n_geo:] == 0).all()
    else:
        assert (want[:, 0] == gc.SENTINEL16).all() and (want[:, 1 + n_geo:] == gc.SENTINEL16).all()


def test_attr_gather_bwd_rejects_h_layout_without_aligned_columns():
    ops = _ops()
    dh = filled((8, 16), gc.SENTINEL16, torch.float16)
    dxa = filled((8, 96), 1.0, torch.float16)
    for in_pad, n_enc in ((96, 66), (24, 16)):
        with pytest.raises(_err()):
            ops.attr_gather_bwd(None, None, 8, dxa, dxa, in_pad, n_enc, 7, dh, h_layout=True)
    assert (host(dh) == gc.SENTINEL16).all()


def _sigma_inputs(h0):
    h = np.full((h0.size, 16), np.nan, F16)
    h[:, 0] = h0
    return h


def test_sigma_every_fp16_input():
    """X, exhaustive over h0: sigma = exp(h0) within EXP_ULPS fp32 ulps; both adjoints with d_sigma = +-2^k and loss_scale = 128
    (only expf rounds) equal fp16(d * exp(clamp(h0, -15, 15)) * 128); l4d_sigma_bwd_rows, fed with l4d_sigma_from_h's output, is
    bit-equal to l4d_sigma_bwd for every finite h0 (clamping commutes with exp)."""
    ops = _ops()
    x = gc.all_f16()
    P = x.size
    x64 = x.astype(F64)
    h = dev(_sigma_inputs(x))
    sigma_t = ops.sigma_from_h(h)
    sigma = host(sigma_t)
    with np.errstate(over="ignore"):
        v = np.exp(x64)
    fmax, fmin = float(np.finfo(F32).max), 2.0 ** -126
    normal = np.isfinite(x) & (v >= fmin) & (v <= fmax)
    dist = np.abs(sigma[normal].astype(F64) - v[normal]) / np.spacing(v[normal].astype(F32)).astype(F64)
    print(f"l4d_sigma_from_h: largest distance from float64 exp {dist.max():.2f} fp32 ulps over {int(normal.sum())} normal results")
    assert dist.max() <= gc.EXP_ULPS
    over = ~np.isnan(x) & (v > fmax * (1 + 2.0 ** -24))
    under = ~np.isnan(x) & (v < 2.0 ** -150)
    assert over.sum() > 1000 and under.sum() > 1000 and np.isposinf(sigma[over]).all() and (sigma[under] == 0).all()
    sub = ~np.isnan(x) & ~normal & ~over & ~under
    assert (sigma[sub] >= 0).all() and (sigma[sub] <= F32(fmin) * F32(1.0 + 2.0 ** -20)).all()
    assert np.isnan(sigma[np.isnan(x)]).all() and (sigma[x == 0] == 1.0).all() and (x == 0).sum() == 2
    ok = ~np.isnan(x)
    order = np.argsort(x64[ok], kind="stable")
    in_order = sigma[ok][order]
    assert (in_order[1:] >= in_order[:-1]).all(), "sigma not monotone"

    d = gc.sigma_d_pow2(P)
    want64 = gc.trunc_exp_bwd64(np.where(ok, x64, 0.0), d, 128.0)
    dh = filled((P, 16), gc.SENTINEL16, torch.float16)
    ops.sigma_bwd(h, dev(d), 128.0, dh)
    dh = host(dh)
    assert (dh[:, 1:] == gc.SENTINEL16).all(), "l4d_sigma_bwd touches column 0 only"
    n_near, worst = gc.x_check(dh[ok, 0], want64[ok], "l4d_sigma_bwd")
    print(f"l4d_sigma_bwd: {n_near} near-boundary cases, largest distance among differing cases {worst:.2f} fp32 ulps")
    dh2 = filled((P, 16), gc.SENTINEL16, torch.float16)
    ops.sigma_bwd_rows(sigma_t, dev(d), 128.0, dh2)
    dh2 = host(dh2)
    assert_bits(dh2[:, 1:], np.zeros((P, 15), F16), "l4d_sigma_bwd_rows writes +0 in columns 1..15")
    fin = np.isfinite(x)
    assert_bits(dh2[fin, 0], dh[fin, 0], "sigma_bwd_rows(sigma_from_h) == sigma_bwd for every finite h0")
    n_near, worst = gc.x_check(dh2[ok, 0], want64[ok], "l4d_sigma_bwd_rows")
    print(f"l4d_sigma_bwd_rows: {n_near} near-boundary cases, largest distance among differing cases {worst:.2f} fp32 ulps")
    assert np.isposinf(dh[ok, 0]).any() and np.isneginf(dh[ok, 0]).any() and (dh[ok, 0] == 0).any()


@pytest.mark.parametrize("P", gc.SIGMA_SMALL_P)
def test_sigma_small_launches(P):
    """X with no near-boundary case (tests/test_glue_cpu.py): bit-equal.  Below, at and above one workgroup; non-finite d_sigma."""
    ops = _ops()
    h0, d = gc.sigma_small_case(P)
    bad = np.array([np.inf, -np.inf, np.nan], F32)
    if P > 3:
        d = d.copy()
        d[:3] = bad
    h = dev(_sigma_inputs(h0))
    sigma_t = ops.sigma_from_h(h)
    v = np.exp(h0.astype(F64))
    assert (np.abs(host(sigma_t).astype(F64) - v) <= gc.EXP_ULPS * np.spacing(v.astype(F32)).astype(F64)).all()
    want = np.zeros(P, F16)
    good = np.isfinite(d)
    with np.errstate(over="ignore"):
        want[good] = gc.trunc_exp_bwd64(h0[good], d[good], 128.0).astype(F16)
    dh, dh2 = filled((P + 1, 16), gc.SENTINEL16, torch.float16), filled((P + 1, 16), gc.SENTINEL16, torch.float16)
    dd = dev(d)
    ops.call("l4d_sigma_bwd", ops._p(h), ops._p(dd), P, 128.0, ops._p(dh), ops._stream())
    ops.call("l4d_sigma_bwd_rows", ops._p(sigma_t), ops._p(dd), P, 128.0, ops._p(dh2), ops._stream())
    dh, dh2 = host(dh), host(dh2)
    for got, name in ((dh, "l4d_sigma_bwd"), (dh2, "l4d_sigma_bwd_rows")):
        assert_bits(got[:P][good, 0], want[good], name)
        assert not np.isfinite(got[:P][~good, 0]).any(), f"{name}: a non-finite d_sigma stays non-finite"
        assert (got[P] == gc.SENTINEL16).all()
    assert (dh[:P, 1:] == gc.SENTINEL16).all()
    assert_bits(dh2[:P, 1:], np.zeros((P, 15), F16), "columns 1..15")


# =================================================================================================================================
# 4. hex planes with unequal resolutions
# =================================================================================================================================
def _close(got, ref, rtol, atol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance; max abs err {float(err.max()):.3e}, ref max {float(ref.abs().max()):.3e}"


_planes = {}


def _planes_pair():
    """(float64 oracle, HIP module) with the same deterministic parameters; built once."""
    if not _planes:
        from lidar4d_amd.planes_field import Planes4D
        from oracle import fields_ref
        from oracle.detparams import det_uniform
        ref = fields_ref.Planes4D(output_dim=8, resolution=gc.PLANES_RES, multiscale_res=gc.PLANES_MS)
        mod = Planes4D(output_dim=8, resolution=gc.PLANES_RES, multiscale_res=gc.PLANES_MS)
        with torch.no_grad():
            for (name, p), (name2, q) in zip(ref.named_parameters(), mod.named_parameters()):
                assert name == name2 and p.shape == q.shape
                lo, hi = (0.8, 1.2) if name.split(".")[-1] in ("2", "4", "5") else (0.1, 0.5)  # time planes: combs (0,3) (1,3) (2,3)
                p.copy_(det_uniform(tuple(p.shape), "glue:" + name, lo, hi))
                q.copy_(p)
        shapes = [tuple(p.shape[2:]) for p in mod.planes[1]]
        assert shapes == [(30, 18), (36, 18), (5, 18), (36, 30), (5, 30), (5, 36)] and all(h != w for h, w in shapes)
        _planes["pair"] = (ref.double(), mod.to(DEV))
    return _planes["pair"]


def _planes_reference(xt):
    """Forward, partial forwards and all gradients of the float64 oracle at xt (numpy fp32 [P,4]) for fixed upstream gradients."""
    from oracle.detparams import det_uniform
    ref, _ = _planes_pair()
    P = xt.shape[0]
    gs, gd = det_uniform((P, 16), "glue:gs", -1, 1), det_uniform((P, 16), "glue:gd", -1, 1)
    xr = torch.from_numpy(xt).double().requires_grad_(True)
    for p in ref.parameters():
        p.grad = None
    fs, fd = ref(xr)
    ((fs * gs.double()).sum() + (fd * gd.double()).sum()).backward()
    return dict(fs=fs.detach(), fd=fd.detach(), fs_only=ref.forward_static(xr).detach(), fd_only=ref.forward_dynamic(xr).detach(),
                dxt=xr.grad.clone(), grads=[p.grad.clone() for p in ref.parameters()], gs=gs, gd=gd)


@pytest.mark.parametrize("P", [2049, 1])
def test_planes_unequal_resolutions(P):
    """Planes4D(resolution=(6, 10, 12, 5), multiscale_res=(1, 3)) against oracle.fields_ref.Planes4D in float64, with the
    tolerances of test_planes_vs_reference_golden: every plane has W != H, so a swapped row stride shows."""
    ops = _ops()
    _, mod = _planes_pair()
    xt = gc.planes_xt(P)
    r = _planes_reference(xt)
    for p in mod.parameters():
        p.grad = None
    xg = dev(xt).requires_grad_(True)
    fs, fd = mod(xg)
    _close(fs, r["fs"], 2e-5, 1e-6, "planes static")
    _close(fd, r["fd"], 2e-5, 1e-6, "planes dynamic")
    _close(mod.forward_static(xg), r["fs_only"], 2e-5, 1e-6, "planes static-only")
    _close(mod.forward_dynamic(xg), r["fd_only"], 2e-5, 1e-6, "planes dynamic-only")
    ((fs * r["gs"].to(DEV)).sum() + (fd * r["gd"].to(DEV)).sum()).backward()
    for (name, p), g in zip(mod.named_parameters(), r["grads"]):  # relayout modes 1 (parameters -> arena) and 0 (arena -> gradients)
        _close(p.grad, g, 1e-4, 1e-4, "planes grad " + name)
    dxt = xg.grad.detach().cpu().double()
    ok = torch.from_numpy(gc.planes_dxt_mask(xt))
    if P > 1:
        assert float(ok.double().mean()) >= 0.95
    _close(dxt[ok], r["dxt"][ok], 1e-4, 1e-4, "planes d/dxt")
    clipped = torch.from_numpy((xt <= 0) | (xt >= 1))
    assert bool((dxt[clipped] == 0).all()) and bool((r["dxt"][clipped] == 0).all()), "clipped coordinates have gradient exactly 0"
    if P > 1:
        assert int(clipped.sum()) > 100
    # want_dxt = False, and relayout mode 2 (gradients += arena) on top of a prefill
    garena = torch.zeros(mod.layout.numel, dtype=torch.float32, device=DEV)
    none = ops.planes_bwd(mod.layout, mod._arena(), xg.detach().contiguous(), 0, r["gs"].to(DEV).contiguous(), r["gd"].to(DEV).contiguous(),
                          garena, False)
    assert none is None
    acc = [torch.full_like(p, 0.5) for p in mod._flat_planes()]
    ops.planes_relayout(mod.layout, acc, garena, to_channel_last=False, accumulate=True)
    for (name, _), a, g in zip(mod.named_parameters(), acc, r["grads"]):
        _close(a, g + 0.5, 1e-4, 1e-4, "planes accumulated grad " + name)
