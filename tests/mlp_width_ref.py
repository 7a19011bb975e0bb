"""The integer lattice of tests/mlp_exact_ref.py for any hidden width: the inputs on which the width-generic fused MLP kernels
(csrc/mlp_width.hip, widths 16 / 32 / 128) have to equal a float64 evaluation bit for bit.

Everything that makes the lattice exact -- integer inputs and dy, sparse +-1 weights, a power-of-two inv_loss_scale, and the
``strict`` assertions that every product, every partial sum in any order and every fp16 / fp32 rounding is a no-op -- is
mlp_exact_ref's, imported and used as it is.  Only the shapes are this module's:

  weights: W1 [hidden, in_pad], (n_hidden - 1) x [hidden, hidden], Wo [16, hidden], concatenated row-major;
  non-zeros per row: W1 max(4, ceil(in_pad / hidden)) (a narrow layer needs that many to reach every input column), hidden
  layers 4, Wo max(8, ceil(hidden / 16)); amplitude 2.
"""
import functools

import numpy as np
import torch

from mlp_exact_ref import (_seed, _sums_exact, backward, fits16, fits32, forward, lattice_ints, sparse_pm1, t16,  # noqa: F401
                           t32)

OUT = 16
WIDTHS = (16, 32, 128)
IN_PADS = (16, 32, 64, 96, 128, 160, 176, 192)
SHAPES = [(hidden, in_pad, n_hidden) for hidden in WIDTHS for in_pad in IN_PADS for n_hidden in (1, 2, 3)]  # all 72


def lattice_weights(hidden, in_pad, n_hidden, seed=0):
    rng = _seed(3, hidden, in_pad, n_hidden, seed)
    Ws = [sparse_pm1(hidden, in_pad, max(4, -(-in_pad // hidden)), rng)]
    for _ in range(n_hidden - 1):
        Ws.append(sparse_pm1(hidden, hidden, 4, rng))
    Ws.append(sparse_pm1(OUT, hidden, max(8, -(-hidden // 16)), rng))
    return Ws


def pack(Ws):
    flat = np.concatenate([W.reshape(-1) for W in Ws])
    assert fits16(flat)
    return flat.astype(np.float16)


def n_params(hidden, in_pad, n_hidden):
    return hidden * in_pad + (n_hidden - 1) * hidden * hidden + OUT * hidden


def check_stats(act, dW, hidden, in_pad, n_hidden):
    """The lattice exercises the network: 25 % .. 75 % of every hidden layer active, at least half of every dW block non-zero."""
    for l in range(n_hidden):
        share = float((act[l] > 0).mean())
        assert 0.25 <= share <= 0.75, f"hidden layer {l}: active share {share:.3f}"
    off = 0
    for l, n in enumerate([hidden * in_pad] + [hidden * hidden] * (n_hidden - 1) + [OUT * hidden]):
        nz = float((dW[off:off + n] != 0).mean())
        assert nz >= 0.5, f"dW block {l}: only {nz:.3f} non-zero"
        off += n


class Case:
    """One lattice problem with its reference results (strict: asserted exact); float64 numpy, never modified afterwards."""

    def __init__(self, hidden, in_pad, n_hidden, P, amp=2, seed=0, x=None, Ws=None, dy=None):
        self.hidden, self.in_pad, self.n_hidden, self.P = hidden, in_pad, n_hidden, P
        self.Ws = lattice_weights(hidden, in_pad, n_hidden, seed) if Ws is None else Ws
        self.x = lattice_ints((P, in_pad), amp, (hidden, in_pad, n_hidden, P, seed, 0)) if x is None else x
        self.dy = lattice_ints((P, OUT), amp, (hidden, in_pad, n_hidden, P, seed, 1)) if dy is None else dy
        self.y, self.act = forward(self.x, self.Ws)
        self.dx, self.dW = backward(self.x, self.act, self.dy, self.Ws)
        for a in (self.x, self.dy, self.y, self.act, self.dx, self.dW):
            a.setflags(write=False)

    def stats_ok(self):
        check_stats(self.act, self.dW, self.hidden, self.in_pad, self.n_hidden)

    def grad(self, n=None, inv_loss_scale=1.0):
        """dW over the first n rows only."""
        if n is None or n >= self.P:
            return self.dW * inv_loss_scale
        return backward(self.x[:n], self.act[:, :n], self.dy[:n], self.Ws, inv_loss_scale)[1]

    def w16(self):
        return torch.from_numpy(pack(self.Ws))


CACHE_MAX_ROWS = 4096


@functools.lru_cache(maxsize=None)
def _small_case(hidden, in_pad, n_hidden, P, amp, seed):
    return Case(hidden, in_pad, n_hidden, P, amp, seed)


def case(hidden, in_pad, n_hidden, P, amp=2, seed=0):
    """The lattice case of these parameters; the small ones are computed once per process and shared."""
    if P > CACHE_MAX_ROWS:
        return Case(hidden, in_pad, n_hidden, P, amp, seed)
    return _small_case(hidden, in_pad, n_hidden, P, amp, seed)
