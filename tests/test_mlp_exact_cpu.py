"""The exact-arithmetic lattice of tests/mlp_exact_ref.py, checked without a GPU: its own exactness conditions hold for every
(in_pad, n_hidden) the MLP dispatch instantiates, and the rounding-point oracle (oracle.tcnn_ref.Network in tcnn mode, whose
rounding points are no-ops on the lattice) gives the same y, dx and dW bit for bit."""
import numpy as np
import pytest
import torch

import mlp_exact_ref as mx
from oracle import tcnn_ref

LARGE_P = 131109  # the grid-stride row count of tests/test_gpu_mlp_exact.py


@pytest.mark.parametrize("in_pad,n_hidden", mx.SHAPES)
def test_lattice_is_exact(in_pad, n_hidden):
    """Constructing a Case runs the strict reference: every fp16 / fp32 round trip and the 2^24 bound are asserted inside."""
    for P in (131, 33):
        c = mx.case(in_pad, n_hidden, P)
        c.stats_ok()
        assert c.y.shape == (P, 16) and c.act.shape == (n_hidden, P, 64) and c.dx.shape == (P, in_pad)
        assert c.dW.shape == (mx.n_params(in_pad, n_hidden),)
        assert np.abs(c.y).max() > 0 and np.abs(c.dx).max() > 0
        # a prefix of the rows: same per-row results, its own dW
        assert np.array_equal(c.grad(P), c.dW) and not np.array_equal(c.grad(P - 1), c.dW)
        assert np.array_equal(c.grad(0), np.zeros_like(c.dW))
        assert np.array_equal(c.grad(P, 1.0 / 128) * 128, c.dW)


@pytest.mark.parametrize("in_pad,n_hidden", [(16, 2), (96, 2), (192, 3)])
def test_large_lattice_is_exact(in_pad, n_hidden):
    c = mx.case(in_pad, n_hidden, LARGE_P, amp=1)
    c.stats_ok()


def test_lattice_weights_are_bounded():
    for in_pad, n_hidden in mx.SHAPES:
        Ws = mx.lattice_weights(in_pad, n_hidden)
        assert [W.shape for W in Ws] == [(64, in_pad)] + [(64, 64)] * (n_hidden - 1) + [(16, 64)]
        for W in Ws:
            assert set(np.unique(W)) <= {-1.0, 0.0, 1.0}
            assert np.abs(W).sum(1).max() <= 8 and 1 <= np.abs(W).sum(0).min() and np.abs(W).sum(0).max() <= 16
        assert mx.pack(Ws).shape == (mx.n_params(in_pad, n_hidden),)


def test_strict_reference_rejects_inexact_inputs():
    c = mx.case(16, 1, 33)
    tiny = [c.Ws[0] * 2.0 ** -13, c.Ws[1]]
    with pytest.raises(AssertionError):
        mx.forward(c.x * (1.0 + 2.0 ** -12), c.Ws)           # x no fp16 number
    with pytest.raises(AssertionError):
        mx.forward(c.x * 2.0 ** -13, tiny)                    # hidden activations underflow fp16
    with pytest.raises(AssertionError):
        mx.backward(c.x, c.act, c.dy * 2.0 ** 14, c.Ws)       # dz leaves the fp16 range
    with pytest.raises(AssertionError):
        mx.backward(c.x, c.act, c.dy, c.Ws, inv_loss_scale=1.0 / 100)
    y, act = mx.forward(c.x * 2.0 ** -13, tiny, strict=False)  # non-strict: rounded where the kernel rounds
    assert mx.fits16(act) and mx.fits16(y) and (act == 0).any() and act.max() <= 2.0 ** -22


@pytest.mark.parametrize("in_pad,n_hidden", mx.SHAPES)
def test_lattice_equals_rounding_point_oracle(in_pad, n_hidden, tcnn_oracle):
    c = mx.case(in_pad, n_hidden, 131)
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64,
           "n_hidden_layers": n_hidden}
    net = tcnn_ref.Network(in_pad, 16, cfg)
    with torch.no_grad():
        net.params.copy_(c.w16().float())
    x = mx.t32(c.x).requires_grad_(True)
    y = net(x)
    assert y.dtype == torch.float16 and torch.equal(y.detach(), mx.t16(c.y))
    y.float().backward(mx.t32(c.dy))
    assert torch.equal(x.grad, mx.t32(c.dx))
    assert torch.equal(net.params.grad, mx.t32(c.dW))
