"""CPU side of the hex-plane widths 4 and 16 (liblidar4d_planes.so; its C ABI checks are tests/test_abi_cpu.py's): the float64 yardstick of
tests/planes_width_ref.py agrees with oracle/fields_ref.py composed as ``fields_ref.LiDAR4D.density`` composes it (so that it is
pinned before tests/test_gpu_planes_width.py lets it judge a kernel); ``LiDAR4D(n_features_per_level_plane = 4 / 16)`` constructs
with the oracle's state-dict keys and shapes, without the fused pipeline, and what cannot run is refused by name.  No GPU."""
import pytest
import torch

import planes_width_ref as pw
import test_abi_cpu as abi
from oracle import fields_ref
from oracle.detparams import det_uniform
from oracle.make_golden import SMALL_MODEL

CFG4 = dict(SMALL_MODEL, n_features_per_level_plane=4, n_levels_plane=4)  # 2 * 4 * 4 + 28 = 60 -> 64 columns
CFG16 = dict(SMALL_MODEL, n_features_per_level_plane=16)                  # 2 * 2 * 16 + 28 = 92 -> 96 columns


# Kept under their earlier names, as calls of the checks in tests/test_abi_cpu.py, which run there for every library: a new library
# adds no test of this kind.
def test_planes_ctypes_signatures_match_header_prototypes():
    abi.test_ctypes_signatures_match_header_prototypes(abi.ROW["planes"])


def test_planes_library_exports_no_name_of_another():
    abi.test_no_library_exports_a_name_of_another()


# ---- the float64 yardstick against the oracle ------------------------------------------------------------------------------
def _close(got, want, tol, what):
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(((got - want).abs() / (1.0 + want.abs())).max())
    assert err <= tol, (what, err)


def _oracle_density_planes(pl, xt, flow, frame):
    """The plane lines of fields_ref.LiDAR4D.density (oracle/fields_ref.py:341-363) on a Planes4D of its own."""
    x, nf = xt[:, :3], pw.NUM_FRAMES
    plane_s, plane_d = pl(xt)
    plane_1 = plane_2 = plane_d
    if frame < nf - 1:
        t1 = torch.tensor((frame + 1) / nf)
        plane_1 = pl.forward_dynamic(torch.cat([x + flow[:, :3], t1.expand(x.shape[0], 1)], -1))
    if frame > 0:
        t2 = torch.tensor((frame - 1) / nf)
        plane_2 = pl.forward_dynamic(torch.cat([x + flow[:, 3:], t2.expand(x.shape[0], 1)], -1))
    return plane_s, 0.5 * plane_d + 0.25 * (plane_1 + plane_2)


def _case(C, frame, multiscale, P=300):
    """The oracle runs in float64 here: in fp32 its own rounding of a position near 63 (3.8e-6 a step, times a slope of order one) is
    above the 1e-6 the comparison asks for.  It forms ``x + flow`` itself, in its own precision, where the yardstick takes the fp32
    sum: the drawn coordinates and flows are therefore multiples of 2^-12 (their sum is exact in both), and the fixed rows -- texel
    centres are no such multiples -- get a zero flow."""
    pl = pw.fill_planes(fields_ref.Planes4D(output_dim=C, resolution=pw.RESOLUTION, multiscale_res=multiscale), f"cpu{C}")
    xt, flow = pw.sample_inputs(P, multiscale, key=f"cpu{C}.{frame}")
    n = pw.n_fixed_rows()
    xt[n:], flow[n:] = torch.round(xt[n:] * 4096) / 4096, torch.round(flow[n:] * 4096) / 4096
    flow[:n] = 0.0
    t = torch.tensor([[frame / 50]])
    tinfo = pw.time_info(float(t), pw.NUM_FRAMES)
    assert int(t.reshape(1, 1).float() * (pw.NUM_FRAMES - 1)) == frame and tinfo[3:] == (frame < 50, frame > 0)
    xt[:, 3] = t.reshape(())
    return pl.double(), xt, flow, tinfo


@pytest.mark.parametrize("frame", [0, 25, 50])
@pytest.mark.parametrize("C", [4, 8, 16])
def test_reference_equals_the_oracles_density_composition(C, frame):
    """Forward within 1e-6 of the oracle on every row, texel centres, borders and clipped coordinates included."""
    for multiscale in pw.SCALES:
        pl, xt, flow, tinfo = _case(C, frame, multiscale)
        planes = [list(coefs) for coefs in pl.planes]
        want_s, want_d = _oracle_density_planes(pl, xt.double(), flow.double(), frame)
        got_s, got_d = pw.density_fwd(planes, xt, flow, tinfo)
        _close(got_s, want_s, 1e-6, "plane_s"), _close(got_d, want_d, 1e-6, "plane_d")
        # the sampler alone, all three `which`
        s, d = pw.planes_fwd(planes, xt, 0)
        _close(s, want_s, 1e-6, "planes_fwd static"), _close(d, pl.forward_dynamic(xt.double()), 1e-6, "planes_fwd time")
        assert pw.planes_fwd(planes, xt, 1)[1] is None and pw.planes_fwd(planes, xt, 2)[0] is None
        assert torch.equal(pw.planes_fwd(planes, xt, 1)[0], s) and torch.equal(pw.planes_fwd(planes, xt, 2)[1], d)


@pytest.mark.parametrize("frame", [0, 25, 50])
@pytest.mark.parametrize("C", [4, 8, 16])
def test_reference_adjoint_equals_the_oracles_autograd(C, frame):
    """The analytic adjoint against autograd through the oracle run in float64, within 1e-6 (it agrees to rounding): every plane
    gradient and dflow / dxt.  A sample exactly on a texel centre sits on a kink of the coordinate gradient, where the yardstick
    takes the slope of the cell fp32 selects (tests/planes_width_ref.py) and float64 arithmetic may select the neighbour: d/dxt and
    dflow are compared on the rows off the kinks, and those rows alone carry an output gradient."""
    multiscale = pw.SCALES[1]
    pl, xt, flow, tinfo = _case(C, frame, multiscale)
    planes = [list(coefs) for coefs in pl.planes]
    n_out = len(multiscale) * C
    gs, gd = det_uniform((xt.shape[0], n_out), "cpu.gs", -1, 1).double(), det_uniform((xt.shape[0], n_out), "cpu.gd", -1, 1).double()
    keep = torch.ones(xt.shape[0], dtype=torch.bool)
    keep[:pw.n_fixed_rows()] = False
    keep[3] = True  # (a clipped row off every texel centre with zero flow)
    # (a kink row's weights, taken in the neighbouring cell, differ by fp32's rounding of the position, some 1e-6: those rows get no
    # output gradient here, so that the plane gradients compare to float64 rounding; their values are compared in the forward test)
    gs[~keep], gd[~keep] = 0.0, 0.0
    xt64, flow64 = xt.double().requires_grad_(True), flow.double().requires_grad_(True)
    want_s, want_d = _oracle_density_planes(pl, xt64, flow64, frame)
    ((want_s * gs).sum() + (want_d * gd).sum()).backward()
    grads, dflow, dxt = pw.density_bwd(planes, xt, flow, tinfo, gs, gd)
    for s, coefs in enumerate(pl.planes):
        for ci, p in enumerate(coefs):
            _close(grads[s][ci], p.grad, 1e-6, f"plane gradient {s}.{ci}")
    _close(dflow[keep], flow64.grad[keep], 1e-6, "dflow")
    # the oracle's xt carries the time column of the frame's own lookup only (t1, t2 are constants), as the yardstick's dxt does
    _close(dxt[keep], xt64.grad[keep], 1e-6, "dxt")
    if frame == 0:
        assert not dflow[:, 3:].any()
    if frame == 50:
        assert not dflow[:, :3].any()
    # the sampler's adjoint alone
    pl.zero_grad()
    xt64 = xt.double().requires_grad_(True)
    s_, d_ = pl(xt64)
    ((s_ * gs).sum() + (d_ * gd).sum()).backward()
    grads, dxt = pw.planes_bwd(planes, xt, 0, gs, gd)
    for s, coefs in enumerate(pl.planes):
        for ci, p in enumerate(coefs):
            _close(grads[s][ci], p.grad, 1e-6, f"planes_bwd gradient {s}.{ci}")
    _close(dxt[keep], xt64.grad[keep], 1e-6, "planes_bwd dxt")


def test_time_info_is_the_oracles_frame_logic():
    for frame in range(51):
        t0, t1, t2, has_fwd, has_bwd = pw.time_info(frame / 50, 51)
        f = int(torch.tensor([[frame / 50]]).float() * 50)
        assert (has_fwd, has_bwd) == (f < 50, f > 0)
        assert t1 == float(torch.tensor((f + 1) / 51)) and t2 == float(torch.tensor((f - 1) / 51)) and t0 == float(torch.tensor(frame / 50))


# ---- constructors ------------------------------------------------------------------------------------------------------------
def _shapes(sd):
    """(the refinement U-Net is not part of the oracle's field model)"""
    return {k: tuple(v.shape) for k, v in sd.items() if not k.startswith("unet.")}


@pytest.mark.parametrize("cfg", [CFG4, CFG16], ids=["C4", "C16"])
def test_model_has_the_oracles_state_dict_and_no_fused_pipeline(cfg, tmp_path):
    from lidar4d_amd import LiDAR4D, checkpoint
    from oracle.detparams import fill_model
    model, ref = fill_model(LiDAR4D(**cfg), seed=7), fields_ref.LiDAR4D(**cfg)
    want = _shapes(ref.state_dict())
    assert _shapes(model.state_dict()) == want
    assert model.fused is False and LiDAR4D(**SMALL_MODEL).fused is True
    C = cfg["n_features_per_level_plane"]
    assert model.planes_encoder.layout.C == C and model.planes_encoder.n_output_dims == ref.planes_encoder.n_output_dims
    assert model.sigma_net.in_pad == {4: 64, 16: 96}[C]
    for p, q in zip(model.planes_encoder.parameters(), ref.planes_encoder.parameters()):
        assert p.shape == q.shape and p.shape[1] == C
    path = checkpoint.save_checkpoint(str(tmp_path / "planes.pth"), model, epoch=2, global_step=5)
    other = LiDAR4D(**cfg)
    info = checkpoint.load_checkpoint(path, other)
    assert info["global_step"] == 5 and not info["missing_keys"] and not info["unexpected_keys"]
    a, b = model.state_dict(), other.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(RuntimeError, match="size mismatch"):  # a checkpoint of another plane width does not load silently
        checkpoint.load_checkpoint(path, LiDAR4D(**SMALL_MODEL))


def test_planes_init_is_the_references():
    from lidar4d_amd.planes_field import Planes4D
    for C in (4, 8, 16):
        mod = Planes4D(output_dim=C, resolution=pw.RESOLUTION, multiscale_res=(1, 2))
        ref = fields_ref.Planes4D(output_dim=C, resolution=pw.RESOLUTION, multiscale_res=(1, 2))
        assert [(n, tuple(p.shape)) for n, p in mod.named_parameters()] == [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
        for s, coefs in enumerate(mod.planes):
            for ci, p in enumerate(coefs):
                a, b = pw.COMBS[ci]
                assert tuple(p.shape) == mod.layout.plane_shape(s, ci) == (1, C, mod.layout.res[s][b], mod.layout.res[s][a])
                if b == 3:
                    assert bool((p == 1).all())
                else:
                    assert 0.1 <= float(p.detach().min()) and float(p.detach().max()) <= 0.5


def test_refusals():
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.planes_field import Planes4D
    for C in (2, 6, 12, 32):
        with pytest.raises(ValueError, match="4, 8 or 16"):
            Planes4D(output_dim=C)
        with pytest.raises(ValueError, match="4, 8 or 16"):
            LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=C))
    with pytest.raises(ValueError, match=r"44 input columns, padded to 48"):  # SMALL_MODEL with C = 4: no MLP kernel of that width
        LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=4))
    with pytest.raises(ValueError, match="n_features_per_level_hash = 4"):  # what still raises in the model
        LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_hash=8))


def test_unfused_model_is_never_captured():
    from lidar4d_amd import LiDAR4D
    from lidar4d_amd.trainer import Trainer
    tr = Trainer.__new__(Trainer)  # graphs_supported() asks the model first
    tr.model = LiDAR4D(**CFG4)
    assert tr.graphs_supported() is False


def test_no_cpu_fallback():
    from lidar4d_amd import ops
    from lidar4d_amd.planes_field import Planes4D
    mod = Planes4D(output_dim=4, resolution=pw.RESOLUTION, multiscale_res=(1,))
    xt, flow = pw.sample_inputs(9, (1,))
    with pytest.raises(Exception, match="no CPU fallback"):
        mod(xt)
    with pytest.raises(Exception, match="no CPU fallback"):
        mod.density_features(xt, flow, torch.zeros(8))
    with pytest.raises(Exception, match="no CPU fallback"):
        ops.planes_fwd(mod.layout, torch.zeros(mod.layout.numel), xt, 0, width_lib=True)
