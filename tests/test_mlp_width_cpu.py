"""CPU side of the hidden widths 16, 32 and 128: the integer lattice of tests/mlp_width_ref.py is exact for all 72 shapes,
``tcnn.Network`` has the oracle's parameter count and layer shapes at every width, and a model of
mixed widths constructs, has the oracle's state-dict keys and shapes and survives a checkpoint round trip.  No GPU."""
import numpy as np
import pytest
import torch

import mlp_width_ref as mw
import test_abi_cpu as abi

MIXED = dict(hidden_dim_sigma=32, hidden_dim_lidar=128, hidden_dim_flow=16)


# ---- the lattice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,in_pad,n_hidden", mw.SHAPES)
def test_lattice_is_exact_and_exercises_the_network(hidden, in_pad, n_hidden):
    """Case() runs the float64 reference with strict=True: every product, sum and rounding of the lattice is exact."""
    for P in (131, 33, 1):
        c = mw.case(hidden, in_pad, n_hidden, P)
        assert c.y.shape == (P, 16) and c.act.shape == (n_hidden, P, hidden) and c.dx.shape == (P, in_pad)
        assert c.dW.shape == (mw.n_params(hidden, in_pad, n_hidden),) == tuple(c.w16().shape)
        if P >= 33:
            c.stats_ok()


@pytest.mark.parametrize("hidden", mw.WIDTHS)
def test_lattice_is_exact_at_the_grid_stride_row_count(hidden):
    """The row counts of tests/test_gpu_mlp_width.py::test_grid_stride: 20,011 and 65,573 rows keep every dW sum below 2^24."""
    for P in (20011, 65573):
        mw.Case(hidden, 96, 2, P).stats_ok()


# Kept under their earlier names, as calls of the checks in tests/test_abi_cpu.py, which run there for every library: a new library
# adds no test of this kind.
def test_mlp_ctypes_signatures_match_header_prototypes():
    abi.test_ctypes_signatures_match_header_prototypes(abi.ROW["mlp"])


def test_mlp_library_exports_no_name_of_another():
    abi.test_no_library_exports_a_name_of_another()


# ---- modules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out,n_hidden", [(120, 16, 1), (87, 1, 2), (16, 6, 2), (176, 16, 3)])
@pytest.mark.parametrize("width", [16, 32, 64, 128])
def test_network_parameters_equal_the_oracles(width, n_in, n_out, n_hidden):
    from lidar4d_amd import tcnn
    from oracle import tcnn_ref
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": n_hidden}
    net, ref = tcnn.Network(n_in, n_out, cfg), tcnn_ref.Network(n_in, n_out, cfg)
    assert net.params.numel() == ref.params.numel()
    assert [tuple(s) for s in net.shapes] == [tuple(s) for s in ref.shapes]
    assert net.n_neurons == width and net.in_pad == ref.shapes[0][1]


def test_unsupported_widths_still_raise():
    from lidar4d_amd import FlowField, tcnn
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 48, "n_hidden_layers": 2}
    with pytest.raises(ValueError, match="n_neurons must be 16, 32, 64 or 128"):
        tcnn.Network(32, 16, cfg)
    with pytest.raises(ValueError, match="hidden 16 / 32 / 64 / 128"):
        FlowField(hidden_dim=256)


def _shapes(sd):
    """(the refinement U-Net is not part of the oracle's field model)"""
    return {k: tuple(v.shape) for k, v in sd.items() if not k.startswith("unet.")}


def test_mixed_width_model_has_the_oracles_state_dict(tmp_path):
    from lidar4d_amd import LiDAR4D, checkpoint
    from oracle import fields_ref
    from oracle.detparams import fill_model
    from oracle.make_golden import SMALL_MODEL
    cfg = dict(SMALL_MODEL, **MIXED)
    model, ref = fill_model(LiDAR4D(**cfg), seed=7), fields_ref.LiDAR4D(**cfg)
    want = _shapes(ref.state_dict())
    assert _shapes(model.state_dict()) == want
    assert model.sigma_net.n_neurons == 32 and model.intensity_net.n_neurons == model.raydrop_net.n_neurons == 128
    assert model.flow_net.hidden_dim == 16 and want["flow_net.mlp.2.weight"] == (16, 16) and want["flow_net.mlp.4.weight"] == (6, 16)
    assert model.flow_net.weight_numel16() == 16 * 16 + 16 * 16 + 16 * 16
    # the flow network's fp16 image in the flat arena is the kernel's layout: [6, h] padded to [16, h] with zeros
    w16 = model.flow_net._weights16()
    assert w16.numel() == model.flow_net.weight_numel16() and not w16[-10 * 16:].any()
    path = checkpoint.save_checkpoint(str(tmp_path / "mixed.pth"), model, epoch=3, global_step=11)
    other = LiDAR4D(**cfg)
    info = checkpoint.load_checkpoint(path, other)
    assert info["epoch"] == 3 and info["global_step"] == 11 and not info["missing_keys"] and not info["unexpected_keys"]
    a, b = model.state_dict(), other.state_dict()
    assert _shapes(b) == want
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(RuntimeError, match="size mismatch"):  # a checkpoint of other widths does not load silently
        checkpoint.load_checkpoint(path, LiDAR4D(**SMALL_MODEL))


def test_width_64_calls_what_it_called():
    """ops.mlp_fwd / mlp_bwd / mlp_fwd_sigma with hidden = 64 (the default) go to liblidar4d_hip.so's entry points, other widths to
    liblidar4d_mlp.so's, and only the default width may skip storing its activations."""
    from lidar4d_amd import ops
    assert ops.mlp_recompute_supported(16, 2) and ops.mlp_recompute_supported(128, 1, 64)
    assert not any(ops.mlp_recompute_supported(i, n, h) for h in mw.WIDTHS for i in mw.IN_PADS for n in (1, 2, 3))
    x = torch.zeros(4, 32, dtype=torch.float16)
    with pytest.raises(Exception, match="no CPU fallback"):
        ops.mlp_fwd(x, x.reshape(-1), 2, hidden=32)
    assert np.prod(mw.case(16, 192, 3, 33).act.shape) == 3 * 33 * 16
