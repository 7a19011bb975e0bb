"""CPU tests of the references in tests/hashgrid_cases.py, which tests/test_gpu_hashgrid_exact.py compares the hash-grid kernels and the
sorted scatter with: the host geometry has the properties the cases rely on, every lattice is exact (the references assert it while
they are evaluated here), the numpy restatement says what the oracle (oracle/tcnn_ref.py, oracle/fields_ref.py) says, and the bound
of the sorted scatter is small enough to see a single record."""
import numpy as np
import pytest
import torch

import hashgrid_cases as hc
from oracle import fields_ref, tcnn_ref

F16, F32, F64 = np.float16, np.float32, np.float64


@pytest.fixture(autouse=True)
def _oracle_modes():
    prev, prev_g = tcnn_ref.get_precision(), tcnn_ref.get_grad_precision()
    tcnn_ref.set_precision("tcnn")
    tcnn_ref.set_grad_precision("fp32")  # gradients in full precision: no fp16 rounding of adjoints or of the accumulation
    yield
    tcnn_ref.set_precision(prev)
    tcnn_ref.set_grad_precision(*prev_g)


# ---- the host geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,F,log2T,L,sizes,hashed", [
    (3, 8, 12, 6, [32, 216, 1728, 4096, 4096, 4096], [0, 0, 0, 1, 1, 1]),
    (3, 4, 14, 6, [32, 216, 1728, 13824, 16384, 16384], [0, 0, 0, 0, 1, 1]),
    (2, 4, 10, 6, [16, 40, 144, 576, 1024, 1024], [0, 0, 0, 0, 1, 1]),
    (2, 8, 12, 6, [16, 40, 144, 576, 2304, 4096], [0, 0, 0, 0, 0, 1]),
    (3, 2, 12, 4, [32, 216, 1728, 4096], [0, 0, 0, 1])])
def test_grid_meta_has_the_lattice_geometry(D, F, log2T, L, sizes, hashed):
    from lidar4d_amd.gridmeta import GridMeta
    geom = hc.Geom(D, F, log2T, L)
    meta = GridMeta(*geom.grid_meta_args())
    assert meta.scale == [2.0, 5.0, 11.0, 23.0, 47.0, 95.0][:L] and meta.res == [3, 6, 12, 24, 48, 96][:L]
    assert meta.size == sizes and [int(h) for h in meta.hashed] == hashed
    for name in ("scale", "res", "size", "offset", "hashed", "n_entries", "n_output_dims"):
        assert getattr(meta, name) == getattr(geom, name), name
    assert all(o % 2 == 0 for o in meta.offset), "the pair loads of F = 4 need even level offsets"
    assert sizes[0] & (sizes[0] - 1) == 0 and sizes[1] & (sizes[1] - 1) and sizes[2] & (sizes[2] - 1)  # dense: a power of two, then `% size`
    for NV, bins in ((2, [0, 0, 0, 2, 2, 2]), (1, [0, 0, 0, 0, 2, 2])) if D == 3 and L == 6 else ():
        if (NV == 2) == (log2T == 12):
            got = [(s >> hc.bs_shift(NV)) if b else 0 for s, b in zip(sizes, hc.binned_levels(geom, NV))]
            assert got == bins, "two bins of the sorted scatter on every hashed level"


def test_coordinates_cover_the_edges():
    x = hc.coords(4159, 3)
    k = x.astype(F64) * 16
    assert (k == np.rint(k)).all() and k.min() == -1 and k.max() == 17 and (k == 0).any() and (k == 16).any()
    geom = hc.Geom(3, 8, 12)
    wrapped = 0
    for lvl in range(6):
        pos = x.astype(F64) * geom.scale[lvl] + 0.5
        wrapped += int((pos < 0).sum())
        if lvl:  # 17/16 lies behind the last vertex (res - 1): its upper corner is vertex number res or res + 1
            assert np.floor(pos).max() + 1 >= geom.res[lvl]
    assert wrapped > 0, "no coordinate wraps through uint32"
    lens = hc.run_lengths(4159)
    ends = np.cumsum(lens)
    assert sum(lens) == 4159 and max(lens) == 70 and min(lens) == 1
    assert (ends % 64 == 0).any() and (ends % 256 == 0).any() and ((ends[:-1] // 64) != ((ends[:-1] - np.asarray(lens[:-1])) // 64)).any()


# ---- the reference against the oracle ---------------------------------------------------------------------------------------------
def oracle_encoding(geom, table16):
    cfg = {"otype": "HashGrid", "n_levels": geom.n_levels, "n_features_per_level": geom.n_features, "log2_hashmap_size": geom.log2T,
           "base_resolution": 3, "per_level_scale": 2.0}
    enc = tcnn_ref.Encoding(geom.n_dims, cfg)
    assert enc.meta["size"] == geom.size and enc.meta["hashed"] == geom.hashed
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(table16.astype(F32)))
    return enc


@pytest.mark.parametrize("D,F", hc.DF)
def test_reference_equals_oracle_encoding(D, F):
    P = 4159
    c = hc.fwd_case(D, F, P)
    enc = oracle_encoding(c["geom"], c["table"])
    out = enc(torch.from_numpy(c["x"]))
    assert out.dtype == torch.float16
    assert hc.same_bits(out.detach().numpy(), c["out16"]).all(), "forward: numpy reference and oracle differ"
    share = hc.needs_rounding(c["v64"])
    print(f"D={D} F={F}: {share:.3f} of the outputs need the fp16 rounding")
    if D == 3:
        assert share > 0.10
    for gs, kind in ((1.0, "scattered"), (128.0, "runs"), (0.25, "scattered")):
        b = hc.bwd_case(D, F, P, kind, gs, False)
        enc.params.grad = None
        out = enc(torch.from_numpy(b["x"]))
        (out.float() * torch.from_numpy((b["dout"] * gs).astype(F32))).sum().backward()
        got, ref = enc.params.grad.numpy().astype(F64), b["ref"].astype(F64)
        assert (np.abs(got - ref) <= 2.0 ** -52 * np.abs(ref)).all(), "table gradient: numpy reference and oracle differ"
    print(f"largest per-entry sum of magnitudes so far: 2^{hc.bwd_ref.largest_log2_units:.1f} units")


@pytest.mark.parametrize("F", [4, 8])
@pytest.mark.parametrize("n_slices,t", hc.T_SETUPS)
def test_reference_equals_oracle_hashgrid_t(F, n_slices, t):
    """The oracle's HashGridT is 2-D.  Forward bit for bit.  Slice gradients: the oracle's adjoint dout * basis * w crosses the fp16
    output of its Encoding (autograd casts it to fp16 there: relative 2^-11 wherever the basis is not a power of two -- the kernels keep
    it in fp32), and its fp32 sums of adjoint * corner weight are not on a lattice: (n + 4) 2^-24 sum |terms| for an element with n terms."""
    P, D = 257, 2
    c = hc.t_fwd_case(D, F, P, n_slices, t)
    geom = c["geom"]
    ref = fields_ref.HashGridT(time_resolution=n_slices, base_resolution=3, max_resolution=96, n_levels=6, n_features_per_level=F,
                               log2_hashmap_size=geom.log2T)
    with torch.no_grad():
        for enc, tab in zip(ref.hash_t, c["tables"]):
            assert enc.meta["size"] == geom.size and enc.meta["scale"] == geom.scale
            enc.params.copy_(torch.from_numpy(tab.astype(F32)))
    out = ref(torch.from_numpy(c["x"]), torch.tensor(t, dtype=torch.float32))
    assert out.dtype == torch.float32
    assert hc.same_bits(out.detach().numpy(), c["out32"]).all(), "forward: numpy reference and oracle differ"
    b = hc.t_bwd_case(D, F, P, n_slices, t)
    out = ref(torch.from_numpy(b["x"]), torch.tensor(t, dtype=torch.float32))
    (out * torch.from_numpy(b["dout"].astype(F32))).sum().backward()
    FO = F // 4
    _, mag, cnt = hc.scatter64(geom, b["x"], b["dout"], FO, want_abs=True)
    i1, i2, w1, w2 = hc.slice_pair_f32(t, n_slices)
    basis = np.abs(hc.lagrange4_f32(t).astype(F64))
    f = np.arange(F)
    for s, enc in enumerate(ref.hash_t):
        want = b["grads_ref"][s].astype(F64) - b["grads0"][s].astype(F64)  # (the reference adds to its prefill in fp32: 2^-24 of the sum)
        if s not in (i1, i2):
            assert enc.params.grad is None and not want.any()
            continue
        w = float(w1 if s == i1 else w2)
        tol = ((2.0 ** -11 + (cnt.reshape(-1, FO)[:, f % FO] + 4) * 2.0 ** -24) * mag.reshape(-1, FO)[:, f % FO] * basis[f // FO][None, :] * w).ravel()
        tol = tol + 2.0 ** -24 * np.abs(b["grads_ref"][s].astype(F64))
        got = enc.params.grad.numpy().astype(F64)
        assert (np.abs(got - want) <= tol).all(), f"slice {s}: numpy reference and oracle differ by up to {np.abs(got - want).max()}"
        assert np.abs(want).max() > 0


def test_time_coefficients():
    assert hc.slice_pair_f32(0.375, 5) == (1, 2, F32(0.5), F32(0.5))
    assert hc.slice_pair_f32(1.0, 5) == (4, 4, F32(1.0), F32(0.0)) and hc.slice_pair_f32(0.3, 1)[:2] == (0, 0)
    b0 = hc.lagrange4_f32(0.0)
    assert b0[0] == 1.0 and not b0[1:].any(), "class B needs a basis that is exactly (1, 0, 0, 0)"
    for t in (0.0, 0.3, 0.375, 1.0):
        want = [float(v) for v in fields_ref.lagrange_basis(torch.tensor(t, dtype=torch.float32))]
        assert [float(v) for v in hc.lagrange4_f32(t)] == want


# ---- every lattice case of the GPU test ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,F", hc.DF)
def test_lattices_are_exact(D, F):
    """The references assert their lattice while they run: evaluate what test_gpu_hashgrid_exact.py will use at its largest sizes."""
    for P in (257, 4159):
        hc.fwd_case(D, F, P)
        for gs in hc.GRAD_SCALES:
            hc.bwd_case(D, F, P, "scattered", gs, True)
        hc.bwd_case(D, F, P, "runs", 1.0, False)
    hc.bwd_case(D, F, 257, "one_cell", 128.0, True)
    if (D, F) in hc.DF_T:
        for n_slices, t in hc.T_SETUPS:
            hc.t_bwd_case(D, F, 4159, n_slices, t, "scattered", 0.25)
            hc.t_bwd_case(D, F, 257, n_slices, t, "runs", 128.0)
    assert hc.bwd_ref.largest_log2_units < 24.0


def test_large_case_draws_every_point():
    rows = hc.big_rows(hc.LEVELS_MIN_POINTS)
    assert np.bincount(rows, minlength=4096).min() > 0 and (rows[1:] != rows[:-1]).mean() > 0.99
    c = hc.t_fwd_big_case()
    assert c["x"].shape == (1 << 18, 3) and c["out16"].shape == (1 << 18, 8) and np.isfinite(c["out16"]).all()


# ---- the sorted scatter's bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,F", hc.SCATTER_DF)
@pytest.mark.parametrize("P", hc.SCATTER_P)
def test_scatter_bound_sees_a_single_record(D, F, P):
    for cloud in hc.SCATTER_CLOUDS:
        r = hc.scatter_case(D, F, P, cloud)
        geom = r["geom"]
        assert sum(r["binned"]) >= 1 and not all(r["binned"])
        for lvl, b in enumerate(r["binned"]):
            sl = geom.level_slice(lvl, F // 4)
            live = cloud != "fx_near_one" or lvl == hc.FX_LEVEL
            assert (r["bound"][sl] > 0).any() == (b and live) and (np.abs(r["ref"][sl]).max() > 0) == live
        print(f"D={D} F={F} P={P} {cloud}: {100 * r['seen']:.2f} % of the contributions to binned levels exceed twice their element's bound")
        if cloud in ("scattered", "runs"):
            assert r["seen"] >= 0.95
        if cloud == "fx_near_one":
            x = r["x"]
            pos = (x[:, 0].astype(F64) * hc.SCALES[hc.FX_LEVEL] + 0.5).astype(F32).astype(F64)
            frac = pos - np.floor(pos)
            assert (frac >= 1 - 2.0 ** -16).all() and (frac < 1).all() and np.floor(pos).max() == 7
            assert np.floor(frac.astype(F32) * F32(32767.0) + F32(0.5)).max() == 32767  # the top of the 15-bit field, and not beyond
            assert (x[1:] != x[:-1]).any(1).all() and r["binned"][hc.FX_LEVEL]
            assert not r["ref"][:geom.offset[hc.FX_LEVEL] * (F // 4)].any()
    # with 4 tiles of 512 rows only 4 of a bin's 8 lists are written: the scattered cloud overflows them; with 16 tiles it does not
    assert hc.list_overflows(geom, F // 4, hc.scatter_case(D, F, P, "scattered")["x"]) == (P == 2048)
    assert hc.EPS_FX < 2.0 ** -15.9
