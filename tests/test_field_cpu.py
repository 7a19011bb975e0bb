"""CPU side of the exact tests of the fused field encode and its adjoint (tests/field_cases.py, tests/test_gpu_field_exact.py): the
float64 reference agrees with oracle/fields_ref.py: LiDAR4D.density under autograd; every GPU case reaches the kernels and task forms it
is there for, and together they reach every launch and branch that arguments alone select; the inputs meet the two conditions under
which the bounds mean something.  No GPU."""
import numpy as np
import pytest
import torch

import field_cases as fc
import hashgrid_cases as hc
from field_cases import F16, F32, F64, U
from oracle import fields_ref, tcnn_ref


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.SPECS), ids=str)
def test_lattice_geometry_is_gridmeta(name):
    from lidar4d_amd.gridmeta import GridMeta
    spec = fc.SPECS[name]
    for g in [spec.hs] + spec.hd:
        m = GridMeta(*g.grid_meta_args())
        assert (m.scale, m.res, m.size, m.offset, m.hashed, m.n_entries) == (g.scale, g.res, g.size, g.offset, g.hashed, g.n_entries)
    assert spec.width <= {4: 64, 8: 96, 16: 192, "6/8": 96}[name]
    # what section 3 of the issue asks of the stacks: dense levels of non-power-of-two size, hashed 2^13 (one window), hashed 2^15
    xy, xz = fc.SPECS[8].hd[0], fc.SPECS[8].hd[1]
    assert not xy.hashed[1] and xy.size[1] == 40 and xy.hashed[7] and xy.size[7] == 1 << 15 and xz.hashed[7] and xz.size[7] == 1 << 13
    assert fc.SPECS[8].hs.hashed[-1] and not fc.SPECS[8].hs.hashed[0] and fc.SPECS[8].hs.size[1] == 216


def test_time_info_covers_what_the_cases_need():
    for frame, nf in fc.FRAMES:
        t, ti, ti8 = fc.frame_info(frame, nf)
        assert (ti[3], ti[4]) == (frame < nf - 1, frame > 0) and ti8[5] == frame
    pair = lambda t: hc.slice_pair_f32(t, 8)[:2]
    assert pair(fc.frame_info(0, 51)[0]) == (0, 0) and pair(fc.frame_info(50, 51)[0]) == (7, 7)  # exactly on a slice: i1 == i2
    ti = fc.frame_info(22, 51)[1]
    assert pair(ti[0]) == (3, 4) and pair(ti[1]) == (3, 4) and pair(ti[2]) == (2, 3)  # a neighbour on another slice pair


# ---- the reference against the oracle ------------------------------------------------------------------------------------------------
ORACLE_SPEC = fc.FieldSpec(8, 8, plane_res=((12, 12, 12, 8), (24, 24, 24, 8)))  # what fields_ref.LiDAR4D builds from (min_resolution 12, 2 scales)


class _GivenFlow(torch.nn.Module):
    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, xt):
        return self.flow


def _oracle(spec, flow):
    m = fields_ref.LiDAR4D(min_resolution=12, base_resolution=3, max_resolution=3 * 2 ** 7, time_resolution=8, n_levels_plane=2,
                           n_levels_hash=8, log2_hashmap_size=11, num_frames=51)
    p = fc.params_of(spec)
    he = m.hash_encoder
    for enc, g in [(he.hash_static, spec.hs)] + [(he.hash_dynamic[i].hash_t[0], spec.hd[i]) for i in range(3)]:
        assert (enc.meta["scale"], enc.meta["size"], enc.meta["hashed"]) == (g.scale, g.size, g.hashed)
    m.planes_encoder.double()
    with torch.no_grad():
        for s, coefs in enumerate(m.planes_encoder.planes):
            for ci, q in enumerate(coefs):
                assert q.shape == p["planes"][s][ci].shape
                q.copy_(p["planes"][s][ci].double())
        he.hash_static.params.copy_(torch.from_numpy(p["hs_table"].astype(F32)))
        for i in range(3):
            for s in range(8):
                he.hash_dynamic[i].hash_t[s].params.copy_(torch.from_numpy(p["hd_tables"][i][s].astype(F32)))
    m.flow_net = _GivenFlow(flow)
    feats = []
    m.sigma_net.register_forward_pre_hook(lambda mod, args: feats.append(args[0]))
    return m, feats


def _oracle_feats(spec, xt, flow16, frame, mode):
    tcnn_ref.set_precision(mode)
    try:
        flow = torch.from_numpy(flow16[:, :6].astype(F64)).requires_grad_(True)
        m, feats = _oracle(spec, flow)
        x = torch.from_numpy(xt[:, :3].astype(F64)) * 2.0 - 1.0  # density() maps it back: (x + bound) / (2 bound), exactly
        m.density(x, torch.tensor(fc.frame_info(frame, 51)[0]))
        return m, feats[0], flow
    finally:
        tcnn_ref.set_precision("tcnn")


@pytest.mark.parametrize("frame", [0, 22, 25, 50])
def test_reference_rows_equal_the_oracles_density_features(frame):
    """Planes and static grid to float64 rounding.  The oracle's HashGridT blends in fp32 (it casts t and the slice features itself): a
    slice blend, four basis terms and the frame blend are at most 12 roundings of partial sums below sum |basis| max |feature| =
    1.7 * 8, so the 2-D x time columns agree within 12 u * 13.6."""
    spec, P = ORACLE_SPEC, 300
    t, tinfo, _ = fc.frame_info(frame, 51)
    xt, flow16 = fc.cloud(P, t, 3)
    _, feats, _ = _oracle_feats(spec, xt, flow16, frame, "tcnn")
    want = feats.detach().double().numpy()
    got = fc.encode_ref(spec, fc.params_of(spec), xt, flow16, tinfo, 96)
    assert want.shape == (P, spec.width) and (got[:, spec.width:] == 1.0).all()
    assert np.abs(got[:, :spec.colsA] - want[:, :spec.colsA]).max() <= 1e-13
    hs = got[:, spec.colsA:spec.colD]  # exact values; the oracle's encoding output is their fp16 (rounding point R2)
    assert (hs.astype(F16).astype(F64) == want[:, spec.colsA:spec.colD]).all() and hc.needs_rounding(hs) > 0.05
    assert np.abs(got[:, spec.colD:spec.width] - want[:, spec.colD:]).max() <= 12 * U * 13.6
    em = fc.dyn_cols(spec, fc.params_of(spec), xt, flow16, tinfo, emulate=True).astype(F64)
    assert np.abs(em - got[:, spec.colD:spec.width]).max() <= 12 * U * 13.6  # the class E emulation is the same function


@pytest.mark.parametrize("frame", [0, 22, 25, 50])
def test_reference_adjoint_equals_the_oracles_autograd(frame):
    """The oracle in its "fp32" mode (no fp16 casts on the way back, which would round the gradients; the hash part is linear, so its
    adjoint does not depend on the rounding of the forward values).  Planes and static table to float64 / exact fp32 sums, dflow to the one fp32 rounding of the oracle's own cast; the
    slice tables within the oracle's own fp32 accumulation (it forms basis * weight * gradient and sums them in fp32)."""
    spec, P = ORACLE_SPEC, 300
    t, tinfo, _ = fc.frame_info(frame, 51)
    xt, flow16 = fc.cloud(P, t, 3)
    dX = fc.make_dX(spec, P, 96, 7)
    m, feats, flow = _oracle_feats(spec, xt, flow16, frame, "fp32")
    (feats.double() * torch.from_numpy(dX[:, :spec.width].astype(F64))).sum().backward()
    arena, hs, hd, dflow = fc.encode_adjoint_ref(spec, fc.params_of(spec), xt, flow16, tinfo, 96, dX, 1.0)
    want = fc.to_arena(spec, [[q.grad for q in coefs] for coefs in m.planes_encoder.planes], F64)
    assert np.abs(arena - want).max() <= 1e-12 * max(1.0, np.abs(want).max()) and np.abs(want).max() > 0.1
    # (density() casts the flow to fp32, so autograd hands its gradient back through an fp32 tensor: one rounding)
    assert (np.abs(dflow - flow.grad.numpy()) <= U * np.abs(dflow) + 1e-13).all()
    assert (dflow[:, :3].any(), dflow[:, 3:].any()) == (bool(tinfo[3]), bool(tinfo[4]))
    assert np.abs(hs - m.hash_encoder.hash_static.params.grad.double().numpy()).max() <= 1e-9
    i1, i2, w1, w2 = hc.slice_pair_f32(tinfo[0], 8)
    basis = np.abs(hc.lagrange4_f32(tinfo[0]).astype(F64))
    for p in range(3):
        # the oracle accumulates an entry's n contributions in fp32: n adds and three products, each one rounding of at most sum |c|
        cols = slice(spec.colD + p * 8, spec.colD + (p + 1) * 8)
        _, mag, cnt = hc.scatter64(spec.hd[p], np.ascontiguousarray(xt[:, list(fc.AXES[p])]), dX[:, cols].astype(F64) * fc.blend_c0(tinfo), 1, want_abs=True)
        for s in range(8):
            g = m.hash_encoder.hash_dynamic[p].hash_t[s].params.grad
            if s not in (i1, i2):
                assert g is None and not hd[p][s].any()  # (and none through the warped lookups: they are no_grad)
                continue
            tol = ((cnt + 3) * U * mag)[:, None] * basis[None, :] * float(w1 if s == i1 else w2)
            assert (np.abs(hd[p][s] - g.double().numpy()) <= tol.reshape(-1)).all() and hd[p][s].any()


# ---- the route map -------------------------------------------------------------------------------------------------------------------
def _fwd_gpu_cases():
    """(spec name, P, scratch, rows, aligned, sigma) of every forward call of tests/test_gpu_field_exact.py."""
    out = []
    for scratch in (False, True):
        for rows in (False, True):
            out += [(8, P, scratch, rows, True, None) for P, _, _ in fc.fwd_combo_cases(scratch)]
    out += [(8, P, True, True, al, None) for al in (True, False) for P, _ in fc.FWD_PAIR_CASES]
    out += [(name, P, s, r, True, None) for name, _ in fc.FWD_OTHER for P, s, r in fc.FWD_OTHER_CASES]
    out += [(name, P, True, True, al, None) for name, al, pts in fc.FWD_BIG_CASES for P in pts]
    out += [(8, fc.FWD_BIG[2], True, True, True, (128, n)) for n in (1, 2)]
    return out


def test_forward_cases_reach_every_launch():
    seen = set()
    for name, P, scratch, rows, aligned, sigma in _fwd_gpu_cases():
        r = fc.fwd_routes(fc.SPECS[name], P, scratch, rows, aligned, sigma)
        seen |= set(r["kernels"])
        if P >= 1 << 18 and scratch and rows:
            assert r["hs_pre"] and r["dh_hs"] == (name == 8)
        if P == (1 << 18) - 1:
            assert not r["hs_pre"] and r["kernels"][-1] == "encode<hdt,rows,hs=2>"  # still gathered
        if P == 8193 and scratch:
            assert r["n_chunks"] == 2
    assert seen == {"warp_coords", "dynhash_fwd_lds", "dynhash_hs_fwd_lds<pair>", "dynhash_hs_fwd_lds<nopair>", "hashgrid_levels_launch",
                    "plane_time_rows", "encode<-,-,hs=0>", "encode<hdt,-,hs=0>", "encode<-,rows,hs=0>", "encode<hdt,rows,hs=0>",
                    "encode<hdt,rows,hs=2>", "encode<hdt,rows,hs=1>", "encode<hdt,rows,hs=1,sigma>", "mlp_fwd_sigma"}
    sig = {n: fc.fwd_routes(fc.SPECS[8], fc.FWD_BIG[2], True, True, True, (128, n))["kernels"][-1] for n in (1, 2)}
    assert sig == {1: "encode<hdt,rows,hs=1,sigma>", 2: "mlp_fwd_sigma"}
    assert fc.FULL % 2 == 1 and np.gcd(fc.FULL, 512) == 1 and fc.FWD_BIG[2] % 512 != 0  # every lane position; a ragged last group of 512


def test_adjoint_cases_reach_every_launch_and_task_form():
    seen, forms = set(), set()
    cases = [(name, in_pad, P, True, True, 0) for name, in_pad in fc.BWD_PREP for P in fc.BWD_POINTS]
    cases += [(name, in_pad, P, r, g, 0) for name, in_pad in fc.BWD_PREP for P in fc.BWD_OTHER_POINTS for r, g in fc.BWD_OTHER_POINTERS]
    cases += [("6/8", 96, P, True, True, 0) for P, _ in fc.BWD_RANGE_CASES] + [(8, 128, n * 64, True, True, 64) for n in fc.BAND_RAYS]
    chunks = set()
    for name, in_pad, P, rows, gd, spr in cases:
        r = fc.bwd_routes(fc.SPECS[name], P, rows, gd, spr, in_pad)
        if P == 0:
            continue
        seen |= set(r["kernels"])
        forms |= {(name, f) for f in r["task_forms"]}
        chunks.add((r["n_chunks"], r["wave_skip"]))
        want_dyn = ("planes_dyn<-,->" if not rows else "planes_dyn<rows,->" if not gd or name == 4 else "planes_dyn_wide" if name == 16 else "planes_dyn<rows,prep>")
        assert want_dyn in r["kernels"], (name, P, rows, gd, r["kernels"])
        assert ("prep<unstaged>" in r["kernels"]) == (name == 4) and ("prep<staged>" in r["kernels"]) == (name != 4 and not (rows and gd))
        assert r["n_chunks"] == (1 if P <= 2048 else min(256, -(-P // 2048))) and r["wave_skip"] == int(spr == 64)
    assert seen == {"bs_scatter", "prep<unstaged>", "prep<staged>", "plane_time_rows", "planes_dyn<-,->", "planes_dyn<rows,->",
                    "planes_dyn<rows,prep>", "planes_dyn_wide", "planes_static", "dynhash_lds", "dynhash_expand"}
    assert {f for n, f in forms if n == 8} == {"generic", "fast", "parity"}
    assert {f for n, f in forms if n == "6/8"} >= {"generic-range", "fast-range"}
    assert {c[0] for c in chunks} >= {1, 2, 3, 35}
    r = fc.bwd_routes(fc.SPECS[8], 71680, True, True, 64, 128)  # three chunks of 23,936 with a ragged last one
    assert (r["n_chunks"], r["chunk_ps"], r["n_chunks_ps"], 71680 - 2 * 23936) == (35, 23936, 3, 23808)
    bands = [b for b in r["bands"] if b[:2] == (1, 0)]
    assert bands == [(1, 0, 0, 32), (1, 0, 32, 32)]  # the 64 x 64 plane: two 64 KB row bands
    assert any(b[3] < fc.bwd_routes(fc.SPECS[8], 64, True, True, 0, 128)["bands"][0][3] for b in r["bands"])  # and a ragged band
    r68 = fc.bwd_routes(fc.SPECS["6/8"], 4159, True, True, 0, 96)
    assert [t[3] for t in r68["tasks"] if t[:2] == (0, 6)] == [16384, 16384, 4096] and len([t for t in r68["tasks"] if t[:2] == (0, 7)]) == 4
    assert [t[2] for t in fc.bwd_routes(fc.SPECS[8], 4159, True, True, 0, 128)["tasks"] if t[:2] == (0, 7)] == ["parity", "parity"]


def test_ray_cloud_is_what_the_band_skip_needs():
    xt, _ = fc.ray_cloud(64, 0.5)
    seg = xt[:, :3].reshape(64, 64, 3)
    d = np.diff(seg, axis=1)
    assert (((d >= 0).all(1)) | ((d <= 0).all(1))).all()  # every coordinate monotone along a 64-sample segment
    row = lambda y: np.floor(np.asarray(y, F32) * F32(63.0))
    assert row(seg[0, :, 1]).max() == 30 and row(seg[1, :, 1]).min() == 32  # taps rows 30, 31 (band 0 only) / 32, 33 (band 1 only)
    assert (row(seg[2, :, 1]) == 31).all() and seg[2, 0, 1] < seg[2, -1, 1]  # taps rows 31 and 32: the segment ends on both sides of the edge


# ---- the conditions under which the bounds mean something -----------------------------------------------------------------------------
def test_at_most_one_percent_of_plane_elements_may_use_the_midpoint_allowance():
    shares = {}
    for name, frame, nf in [(8, f, n) for f, n in fc.FRAMES] + [(n, 25, 51) for n, _ in fc.FWD_OTHER]:
        c = fc.fwd_case(name, frame, nf)
        shares[(name, frame, nf)] = c["near_share"]
        assert c["near_share"] <= 0.01, (name, frame, nf, c["near_share"])
        v = c["row"][:, c["spec"].colsA:c["spec"].colD]
        assert hc.needs_rounding(v) > 0.05  # the static columns are not all fp16 numbers anyway
    print("[field-cpu] share of plane elements within E of an fp16 midpoint:", min(shares.values()), "-", max(shares.values()))


@pytest.mark.parametrize("name,in_pad", fc.BWD_PREP + (("6/8", 96),), ids=["L4", "L8", "L16", "L6-8"])
def test_contributions_exceed_twice_their_bound(name, in_pad):
    pts = fc.BWD_POINTS if name != "6/8" else [P for P, _ in fc.BWD_RANGE_CASES]
    seen = {}
    for i, P in enumerate(pts):
        (frame, nf), ps = fc.bwd_args(i) if name != "6/8" else (fc.BWD_RANGE_CASES[i][1], 1.0)
        if P:
            seen[P] = fc.bwd_case(name, P, frame, nf, in_pad, ps)["seen"]
            assert seen[P] >= 0.95, (P, seen[P])
    print("[field-cpu] share of contributions above twice their bound:", min(seen.values()), "-", max(seen.values()))


@pytest.mark.parametrize("n_rays", fc.BAND_RAYS)
def test_ray_contributions_exceed_twice_their_bound(n_rays):
    c = fc.band_case(n_rays)
    print("[field-cpu] rays:", n_rays, "share", c["seen"])
    assert c["seen"] >= 0.95 and c["route"]["wave_skip"] == 1
