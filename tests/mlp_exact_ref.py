"""An integer lattice on which the fused MLP kernels (csrc/mlp.hip) have to be EXACT, and its float64 reference.

Inputs and dy are small integers, the weights are sparse +-1 matrices with a bounded number of non-zeros per row and per
column, inv_loss_scale is a power of two.  Then every product is an integer, every partial sum of every contraction -- in
any order, atomics included -- is an integer below 2^24 (exact in fp32), and every value the kernels round to fp16 is an
integer below 2048 (exact in fp16).  A correct kernel therefore equals the float64 evaluation bit for bit, and an indexing,
tail, gating or double-count error shows as an inequality: no tolerance is involved anywhere.

The reference does not assume any of this: it ASSERTS it at every step (``strict=True``), so that a change of the lattice
that breaks exactness fails here, on the CPU, and not as a mysterious mismatch on the GPU.

Weight layout of mlp.hip: W1 [64, in_pad], (n_hidden - 1) x [64, 64], Wo [16, 64], concatenated row-major.
"""
import functools
import math

import numpy as np
import torch

HID, OUT = 64, 16
IN_PADS = (16, 32, 64, 96, 128, 160, 176, 192)
SHAPES = [(in_pad, n_hidden) for in_pad in IN_PADS for n_hidden in (1, 2, 3)]  # every pair the dispatch instantiates
EXACT_SUM = float(1 << 24)  # integers below this are exact in fp32


def _seed(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k) + 12345) % ((1 << 31) - 1)
    return np.random.RandomState(s)


def sparse_pm1(rows, cols, nnz, rng):
    """[rows, cols] with ``nnz`` entries of +-1 per row at columns (stride * r + offset_j) mod cols: circulant-like, so the
    count per column is bounded as well (about nnz * rows / cols), and every column carries at least one entry."""
    stride = -(-cols // rows)
    assert stride <= nnz <= cols
    offs = list(range(stride))
    while len(offs) < nnz:
        o = int(rng.randint(cols))
        if o not in offs:
            offs.append(o)
    W = np.zeros((rows, cols))
    for r in range(rows):
        for o in offs:
            W[r, (stride * r + o) % cols] = 1.0 if rng.randint(2) else -1.0
    assert (np.abs(W).sum(1) == nnz).all() and (np.abs(W).sum(0) >= 1).all()
    return W


def lattice_weights(in_pad, n_hidden, seed=0):
    rng = _seed(1, in_pad, n_hidden, seed)
    Ws = [sparse_pm1(HID, in_pad, 4, rng)]
    for _ in range(n_hidden - 1):
        Ws.append(sparse_pm1(HID, HID, 4, rng))
    Ws.append(sparse_pm1(OUT, HID, 8, rng))
    return Ws


def lattice_ints(shape, amp, seed_key):
    """Integers in {-amp .. amp}, uniformly."""
    return _seed(2, *seed_key).randint(-amp, amp + 1, size=shape).astype(np.float64)


def pack(Ws):
    """The flat fp16 weight vector of l4d_mlp_fwd / _bwd (numpy float16)."""
    flat = np.concatenate([W.reshape(-1) for W in Ws])
    assert fits16(flat)
    return flat.astype(np.float16)


def n_params(in_pad, n_hidden):
    return HID * in_pad + (n_hidden - 1) * HID * HID + OUT * HID


def fits16(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore"):
        return bool(np.isfinite(a).all() and (a.astype(np.float16).astype(np.float64) == a).all())


def fits32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.isfinite(a).all() and (a.astype(np.float32).astype(np.float64) == a).all())


def _sums_exact(A, B):
    """True if no partial sum of A @ B, in any order, can round in fp32: all terms are integers, and for every entry the sum
    of |terms| is below 2^24."""
    if A.size == 0 or B.size == 0:
        return True
    if not ((A == np.rint(A)).all() and (B == np.rint(B)).all()):
        return False
    return float((np.abs(A) @ np.abs(B)).max()) < EXACT_SUM


def forward(x, Ws, strict=True):
    """-> y [P, 16], act [n_hidden, P, 64] (float64).  The hidden activations and y are rounded to fp16 where the kernel rounds
    them; strict: that rounding, and the fp32 accumulation in front of it, must be no-ops."""
    assert fits16(x), "x is an fp16 argument"
    h, acts = x, []
    for l, W in enumerate(Ws):
        z = h @ W.T
        if strict:
            assert _sums_exact(h, W.T) and fits32(z), f"layer {l}: a matmul result does not survive fp32"
        z = z.astype(np.float32).astype(np.float64)
        if l < len(Ws) - 1:
            z = np.maximum(z, 0.0)
        with np.errstate(over="ignore"):
            r = z.astype(np.float16).astype(np.float64)
        if strict:
            assert (r == z).all(), f"layer {l}: a value the kernel rounds to fp16 does not survive fp16"
        h = r
        if l < len(Ws) - 1:
            acts.append(h)
    return h, np.stack(acts)


def backward(x, act, dy, Ws, inv_loss_scale=1.0, strict=True):
    """-> dx [P, in_pad], dW (flat, weight layout, already multiplied by inv_loss_scale) in float64.  ReLU' = act > 0.
    strict: every dz and dx survives fp16, every matmul survives fp32, and for every dW entry sum |dz|^T |h| < 2^24."""
    m, e = math.frexp(inv_loss_scale)
    assert m == 0.5 and -30 < e <= 1, "inv_loss_scale must be a power of two"
    assert fits16(dy), "dy is an fp16 argument"
    n_hidden = len(Ws) - 1
    ins = [x] + [act[l] for l in range(n_hidden)]  # input of layer l
    dz, dWs = dy, [None] * len(Ws)
    for l in range(n_hidden, -1, -1):
        dWs[l] = dz.T @ ins[l]
        dh = dz @ Ws[l]
        if strict:
            assert _sums_exact(dz.T, ins[l]), f"layer {l}: a dW entry's sum of absolute terms reaches 2^24"
            assert _sums_exact(dz, Ws[l]) and fits32(dh), f"layer {l}: dz W does not survive fp32"
            assert fits32(dWs[l] * inv_loss_scale)
        if l > 0:
            dh = np.where(act[l - 1] > 0, dh, 0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            r = dh.astype(np.float32).astype(np.float16).astype(np.float64)
        if strict:
            assert (r == dh).all(), f"layer {l}: a dz / dx value does not survive fp16"
        dz = r
    return dz, np.concatenate([d.reshape(-1) for d in dWs]) * inv_loss_scale


def check_stats(act, dW, in_pad, n_hidden):
    """The lattice exercises the network: 25 % .. 75 % of every hidden layer active, at least half of every dW block non-zero."""
    for l in range(n_hidden):
        share = float((act[l] > 0).mean())
        assert 0.25 <= share <= 0.75, f"hidden layer {l}: active share {share:.3f}"
    off = 0
    for l, n in enumerate([HID * in_pad] + [HID * HID] * (n_hidden - 1) + [OUT * HID]):
        nz = float((dW[off:off + n] != 0).mean())
        assert nz >= 0.5, f"dW block {l}: only {nz:.3f} non-zero"
        off += n


class Case:
    """One lattice problem with its reference results; everything float64 numpy, never modified after construction."""

    def __init__(self, in_pad, n_hidden, P, amp=2, seed=0, x=None, Ws=None, dy=None):
        self.in_pad, self.n_hidden, self.P = in_pad, n_hidden, P
        self.Ws = lattice_weights(in_pad, n_hidden, seed) if Ws is None else Ws
        self.x = lattice_ints((P, in_pad), amp, (in_pad, n_hidden, P, seed, 0)) if x is None else x
        self.dy = lattice_ints((P, OUT), amp, (in_pad, n_hidden, P, seed, 1)) if dy is None else dy
        self.y, self.act = forward(self.x, self.Ws)
        self.dx, self.dW = backward(self.x, self.act, self.dy, self.Ws)
        for a in (self.x, self.dy, self.y, self.act, self.dx, self.dW):
            a.setflags(write=False)

    def stats_ok(self):
        check_stats(self.act, self.dW, self.in_pad, self.n_hidden)

    def grad(self, n=None, inv_loss_scale=1.0):
        """dW over the first n rows only (the per-row results y / act / dx of a prefix are the prefix of the results)."""
        if n is None or n >= self.P:
            return self.dW * inv_loss_scale
        return backward(self.x[:n], self.act[:, :n], self.dy[:n], self.Ws, inv_loss_scale)[1]

    def w16(self):
        return torch.from_numpy(pack(self.Ws))


CACHE_MAX_ROWS = 4096  # larger cases (hundreds of MB of float64) are built for the one test that asks and freed with it


@functools.lru_cache(maxsize=None)
def _small_case(in_pad, n_hidden, P, amp, seed):
    return Case(in_pad, n_hidden, P, amp, seed)


def case(in_pad, n_hidden, P, amp=2, seed=0):
    """The lattice case of these parameters; the small ones are computed once per process and shared."""
    if P > CACHE_MAX_ROWS:
        return Case(in_pad, n_hidden, P, amp, seed)
    return _small_case(in_pad, n_hidden, P, amp, seed)


def t16(a):
    """float64 lattice array -> fp16 torch tensor (exact: asserted)."""
    assert fits16(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float16))


def t32(a):
    assert fits32(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
