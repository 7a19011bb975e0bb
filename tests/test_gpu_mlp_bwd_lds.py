"""The backward MLP kernel's wave-private LDS staging image (csrc/mlp.hip "Backward", csrc/mlp_dev.h BwdStage): the batch-major
operands of every dW contraction -- dy, the hidden activations, x and each layer's dZ -- are written there from the chain layout and
read back transposed.  tests/test_gpu_mlp_exact.py pins the arithmetic on lattice data; here: run-to-run determinism and float64
parity of one macro tile on ordinary data, the region base and the row / feature roles on data that is not symmetric in them, and
non-finite adjoints passing through the image unsaturated.  Run with ``-m gpu`` on an MI355X."""
import ast
import inspect
import textwrap

import numpy as np
import pytest
import torch

import mlp_exact_ref as mx
import test_gpu_ops as gpu_ops_tests

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(16, 2), (96, 2), (128, 1), (192, 3)]  # two waves per SIMD + recompute, prefetching, the density network, two launches


def ops_():
    from lidar4d_amd import ops
    return ops


def _bwd_tolerances():
    """(rtol, atol / max |reference|) of test_mlp_fwd_bwd's "mlp dW" and "mlp dX" comparisons, read from that test itself."""
    tree = ast.parse(textwrap.dedent(inspect.getsource(gpu_ops_tests.test_mlp_fwd_bwd)))
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "id", None) == "rel_close":
            kw = {k.arg: k.value for k in node.keywords}
            what = ast.literal_eval(kw["what"])
            if what in ("mlp dW", "mlp dX"):
                assert isinstance(kw["atol"], ast.BinOp) and isinstance(kw["atol"].op, ast.Mult)
                out[what] = (float(ast.literal_eval(kw["rtol"])), float(ast.literal_eval(kw["atol"].left)))
    assert set(out) == {"mlp dW", "mlp dX"}, out
    return out


def random_problem(in_pad, n_hidden, P, seed):
    """Ordinary fp16 data at the scale test_mlp_fwd_bwd uses (weights +-0.3, inputs and output gradient +-1), as float64."""
    rng = np.random.RandomState(seed)
    r16 = lambda lo, hi, *shape: rng.uniform(lo, hi, size=shape).astype(np.float16).astype(np.float64)
    Ws = [r16(-0.3, 0.3, mx.HID, in_pad)] + [r16(-0.3, 0.3, mx.HID, mx.HID) for _ in range(n_hidden - 1)] + [r16(-0.3, 0.3, mx.OUT, mx.HID)]
    return Ws, r16(-1, 1, P, in_pad), r16(-1, 1, P, mx.OUT)


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float16)).to(DEV)


def run_bwd(x, act, dy, w, n_hidden):
    g = torch.zeros(w.numel(), device=DEV)
    dx = ops_().mlp_bwd(x, act, dy, w, n_hidden, g, 1.0)
    torch.cuda.synchronize()
    return dx, g


def block_of(in_pad, n_hidden, layer):
    """(offset, rows, cols) of layer ``layer`` (0-based) in the flat weight / grad_w vector."""
    sizes = [(mx.HID, in_pad)] + [(mx.HID, mx.HID)] * (n_hidden - 1) + [(mx.OUT, mx.HID)]
    off = sum(r * c for r, c in sizes[:layer])
    return off, sizes[layer][0], sizes[layer][1]


# ---- 1. one macro tile, one flushing wavefront: deterministic, and right ------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 31, 32])
@pytest.mark.parametrize("in_pad,n_hidden", SHAPES)
def test_single_tile_is_deterministic_and_matches_float64(in_pad, n_hidden, P):
    ops = ops_()
    tol = _bwd_tolerances()
    Ws, x64, dy64 = random_problem(in_pad, n_hidden, P, seed=1000 * in_pad + 10 * n_hidden + P)
    w, x, dy = dev16(np.concatenate([W.reshape(-1) for W in Ws])), dev16(x64), dev16(dy64)
    _, act = ops.mlp_fwd(x, w, n_hidden, save_act=True)
    # float64 reference of the backward pass on the activations the kernel is given (fp16 roundings where the kernel has them)
    dx_ref, g_ref = mx.backward(x64, act.double().cpu().numpy(), dy64, Ws, 1.0, strict=False)
    dx_ref, g_ref = torch.from_numpy(dx_ref), torch.from_numpy(g_ref)
    variants = [act] + ([None] if ops.mlp_recompute_supported(in_pad, n_hidden) else [])
    for a in variants:  # saved activations; recomputed ones where that kernel exists
        dx1, g1 = run_bwd(x, a, dy, w, n_hidden)
        dx2, g2 = run_bwd(x, a, dy, w, n_hidden)
        assert torch.equal(dx1, dx2) and torch.equal(g1, g2), "two calls differ"
        print(f"in_pad {in_pad} n_hidden {n_hidden} P {P} recompute {a is None}: max |dW - ref| {float((g1.cpu().double() - g_ref).abs().max()):.3e} "
              f"of {float(g_ref.abs().max()):.3e}, max |dX - ref| {float((dx1.cpu().double() - dx_ref).abs().max()):.3e} of {float(dx_ref.abs().max()):.3e}")
        gpu_ops_tests.rel_close(g1, g_ref, rtol=tol["mlp dW"][0], atol=tol["mlp dW"][1] * float(g_ref.abs().max()), what="mlp dW")
        gpu_ops_tests.rel_close(dx1, dx_ref, rtol=tol["mlp dX"][0], atol=tol["mlp dX"][1] * float(dx_ref.abs().max()), what="mlp dX")


# ---- 2. wave-private regions; rows and features are not interchangeable ----------------------------------------------------------
@pytest.mark.parametrize("in_pad,n_hidden", SHAPES)
def test_one_hot_rows_reach_the_right_dw_entries(in_pad, n_hidden):
    """P = 128 + 5: five macro tiles, so the four wavefronts of the first workgroup stage at once.  Row r of the first hidden
    activations carries a value only in feature r % 64 (and x only in column r % in_pad): column k of the dW of layer 1 (the
    layer fed by the first hidden activations) is a sum over the rows r = k (mod 64) alone, while its rows (the layer's dZ, gated
    by the dense later activations) are not restricted -- the block is not symmetric.  Integer data: exact."""
    P = 128 + 5
    Ws = mx.lattice_weights(in_pad, n_hidden, seed=3)
    r = np.arange(P)
    act = mx.lattice_ints((n_hidden, P, mx.HID), 2, (in_pad, n_hidden, P, 78)).clip(0, None)  # dense, about 40 % open gates
    act[0] = 0.0
    act[0, r, r % mx.HID] = 1 + r % 3
    x = np.zeros((P, in_pad))
    x[r, r % in_pad] = 1 + r % 2
    dy = mx.lattice_ints((P, mx.OUT), 2, (in_pad, n_hidden, P, 77))
    dx_ref, g_ref = mx.backward(x, act, dy, Ws, 1.0, strict=True)
    dx, g = run_bwd(mx.t16(x).to(DEV), mx.t16(act).to(DEV), mx.t16(dy).to(DEV), torch.from_numpy(mx.pack(Ws)).to(DEV), n_hidden)
    off, rows, cols = block_of(in_pad, n_hidden, 1)
    got = g[off:off + rows * cols].view(rows, cols).cpu()
    # the expected block, from its definition: dz of layer 1 (for a single hidden layer: dy itself) against the one-hot rows
    want = torch.from_numpy(g_ref[off:off + rows * cols].reshape(rows, cols))
    if n_hidden == 1:
        by_hand = np.zeros((rows, cols))
        for row in range(P):
            by_hand[:, row % mx.HID] += dy[row] * (1 + row % 3)
        assert np.array_equal(by_hand, want.numpy())
    assert int((want != 0).sum()) > cols, "the expected block is all but empty"
    assert torch.equal(got != 0, want != 0), "non-zeros of the layer-1 dW"
    assert torch.equal(g.cpu(), mx.t32(g_ref)) and torch.equal(dx.cpu(), mx.t16(dx_ref))


# ---- 3. non-finite adjoints pass through the image ----------------------------------------------------------------------------
@pytest.mark.parametrize("in_pad,n_hidden", SHAPES)
def test_infinite_dy_stays_in_its_row(in_pad, n_hidden):
    ops = ops_()
    P, bad = 128 + 5, 70
    Ws, x64, dy64 = random_problem(in_pad, n_hidden, P, seed=5000 + in_pad + n_hidden)
    w, x, dy = dev16(np.concatenate([W.reshape(-1) for W in Ws])), dev16(x64), dev16(dy64)
    dy[bad, 3] = float("inf")
    _, act = ops.mlp_fwd(x, w, n_hidden, save_act=True)
    assert bool((act[:, bad] > 0).any(dim=1).all()), "the row has no open ReLU gate"
    variants = [act] + ([None] if ops.mlp_recompute_supported(in_pad, n_hidden) else [])
    for a in variants:
        dx, g = run_bwd(x, a, dy, w, n_hidden)
        finite_rows = torch.isfinite(dx).all(dim=1).cpu()
        assert not bool(finite_rows[bad]), "dx of the row that carries the infinity is finite"
        others = torch.ones(P, dtype=torch.bool)
        others[bad] = False
        assert bool(finite_rows[others].all()), "the infinity leaked into other rows of dx"
        off, rows, cols = block_of(in_pad, n_hidden, n_hidden)
        assert not bool(torch.isfinite(g[off:off + rows * cols]).all()), "grad_w of the output layer is finite"
