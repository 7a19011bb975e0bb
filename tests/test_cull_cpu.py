"""CPU side of training on culled samples (``render(..., cull=eps, slab=S)``, lidar4d_amd/cull.py): what the option cannot do is
refused by name before anything touches a device, ``early_stop`` under grad keeps its own refusal, the map from compact slab-major rows
to dense sample indices is pinned against a numpy restatement, and a ``Trainer`` with ``cull`` set does not capture its steps.  No GPU."""
import inspect
import types

import numpy as np
import pytest
import torch

from oracle.make_golden import SMALL_MODEL, test_rays as make_rays

TIME = 0.5


def _cpu_call(model, **kw):
    ro, rd = make_rays(5, 3)
    return model.render(ro, rd, torch.tensor([[TIME]]), num_steps=32, **kw)


# ---- refusals that need no device --------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    from lidar4d_amd import LiDAR4D
    model = LiDAR4D(**SMALL_MODEL)
    assert torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())
    for bad in (-1e-6, float("nan"), float("inf"), "1e-4", True):
        with pytest.raises(ValueError, match="cull must be"):
            _cpu_call(model, cull=bad)
    for bad in (0, -16, 1.5, None, True):
        with pytest.raises(ValueError, match="slab must be a positive int"):
            _cpu_call(model, cull=1e-4, slab=bad)
    with pytest.raises(ValueError, match="cull and early_stop"):
        _cpu_call(model, cull=1e-4, early_stop=1e-4)
    with pytest.raises(ValueError, match="cull and early_stop"):
        _cpu_call(model, cull=0.0, early_stop=0.0, slab=8)
    with pytest.raises(ValueError, match="staged=True"):
        _cpu_call(model, cull=1e-4, staged=True, max_ray_batch=2)
    narrow = LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=4, n_levels_plane=4))
    assert narrow.fused is False
    with pytest.raises(ValueError, match="cull needs the fused pipeline"):
        _cpu_call(narrow, cull=1e-4)
    # without a gradient: grad mode off, or nothing requires grad -- the message points to early_stop
    with torch.no_grad(), pytest.raises(ValueError, match="needs a gradient.*early_stop"):
        _cpu_call(model, cull=1e-4)
    # nothing left to refuse: the march starts -- and has no CPU fallback
    with pytest.raises(Exception, match="no CPU fallback"):
        _cpu_call(model, cull=1e-4, slab=16, perturb=True)
    with pytest.raises(Exception, match="no CPU fallback"):
        _cpu_call(model, cull=0, slab=7)
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="needs a gradient.*early_stop"):
        _cpu_call(model, cull=1e-4)


def test_generic_renderer_refuses_cull():
    from lidar4d_amd.renderer import LiDAR_Renderer
    ro, rd = make_rays(5, 3)
    with pytest.raises(ValueError, match="cull needs the fused pipeline"):
        LiDAR_Renderer().run(ro, rd, torch.tensor([[TIME]]), num_steps=8, cull=1e-4)


def test_early_stop_with_grad_still_raises():
    from lidar4d_amd import LiDAR4D
    model = LiDAR4D(**SMALL_MODEL)
    assert torch.is_grad_enabled()
    with pytest.raises(ValueError, match="requires grad"):
        _cpu_call(model, early_stop=1e-4)
    with pytest.raises(ValueError, match="training on culled samples is not supported"):
        _cpu_call(model, early_stop=1e-4, cull=None)
    with torch.no_grad(), pytest.raises(ValueError, match="perturb=True"):
        _cpu_call(model, early_stop=1e-4, perturb=True)


def test_without_the_option_nothing_of_the_march_is_called(monkeypatch):
    """``cull=None`` (the default everywhere) never reaches cull.run; with the option set ``RenderFn.apply`` is not called and the
    result has the march's two extra keys."""
    from lidar4d_amd import LiDAR4D, cull, lidar4d
    calls = []

    def seven(N, num_steps):
        return (torch.zeros(N), torch.zeros(N, 2), torch.zeros(N), torch.zeros(N, num_steps), torch.zeros(N, num_steps),
                torch.zeros(N * num_steps, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))

    def fake_apply(model, rays_o, rays_d, t_dev, noise, num_steps, train, *params):
        calls.append(("apply", rays_o.shape[0], num_steps, train))
        return seven(rays_o.shape[0], num_steps)

    def fake_run(model, rays_o, rays_d, t_dev, noise, num_steps, eps, S, params):
        calls.append(("cull", rays_o.shape[0], num_steps, eps, S, noise is not None, len(params) > 0))
        N = rays_o.shape[0]
        return seven(N, num_steps) + (torch.tensor(N * num_steps), torch.full((N,), num_steps, dtype=torch.int32))

    monkeypatch.setattr(lidar4d.RenderFn, "apply", staticmethod(fake_apply))
    monkeypatch.setattr(cull, "run", fake_run)
    model = LiDAR4D(**SMALL_MODEL)
    ro, rd = make_rays(5, 3)
    t = torch.tensor([[TIME]])
    plain = model.render(ro, rd, t, num_steps=32)
    model.render(ro, rd, t, num_steps=32, cull=None, slab=16)
    assert calls == [("apply", 5, 32, True)] * 2
    del calls[:]
    out = model.render(ro, rd, t, num_steps=32, cull=1e-4)
    assert calls == [("cull", 5, 32, 1e-4, 96, False, True)]  # (slab's default, shared with early_stop)
    assert set(out) == set(plain) | {"evaluated_samples", "retired_at"}
    del calls[:]
    model.render(ro, rd, t, num_steps=32, cull=0.0, slab=64, perturb=True, noise=torch.rand(5, 32))
    assert calls == [("cull", 5, 32, 0.0, 64, True, True)]


# ---- the row map ----------------------------------------------------------------------------------------------------------------
def _row_map_numpy(live_lists, T, S):
    """Compact row -> dense flat index, written out: slab k holds samples k * S .. min((k + 1) * S, T) - 1 of the rays live in front of
    it, ray after ray."""
    out = []
    for k, live in enumerate(live_lists):
        for r in live:
            for s in range(k * S, min((k + 1) * S, T)):
                out.append(int(r) * T + s)
    return np.asarray(out, np.int64)


@pytest.mark.parametrize("T,S,lists", [
    (96, 32, [[0, 1, 2, 3, 4, 5, 6], [0, 2, 3, 6], [6]]),           # shrinks unevenly
    (100, 32, [[0, 1, 2, 3, 4], [1, 2, 4], [1, 4], [4]]),           # a partial last slab (4 samples)
    (100, 32, [[3, 5], [5], [5], [5]]),
    (64, 64, [[0, 1, 2]]),                                          # one slab
    (40, 64, [[2, 0, 1]]),                                          # a slab longer than the ray
    (7, 1, [[0, 1]] * 3 + [[1]] * 4),                               # slabs of one sample
    (96, 32, [[0, 1, 2], [], []]),                                  # an empty list: no rows
    (96, 32, [[]]),
    (96, 32, []),
], ids=["uneven", "partial-last", "partial-last-one-ray", "one-slab", "long-slab", "S1", "empty-behind", "empty", "none"])
def test_row_map_against_numpy(T, S, lists):
    from lidar4d_amd import cull
    want = _row_map_numpy(lists, T, S)
    got = cull.row_map([torch.tensor(l, dtype=torch.int32) for l in lists], T, S)
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert np.array_equal(got.numpy(), want)
    for k, l in enumerate(lists):
        Sp = min(S, T - k * S)
        piece = cull.slab_map(torch.tensor(l, dtype=torch.int32), T, k * S, Sp)
        assert piece.dtype == torch.int64 and np.array_equal(piece.numpy(), _row_map_numpy([[]] * k + [l], T, S))
    if len(want):  # every dense index at most once, all inside [0, N * T)
        assert len(np.unique(want)) == len(want) and want.min() >= 0
    # the backward's order: moving row i to ray_major_position[i] lays the evaluated samples out ray after ray, i.e. sorts the dense
    # indices -- from the rays' retirement points alone, without a sort
    n_rays = 1 + max([max(l) for l in lists if l], default=0)
    at = np.zeros(n_rays, np.int32)
    for k, l in enumerate(lists):
        for r in l:
            at[r] = min((k + 1) * S, T)
    pos = cull.ray_major_position(got, torch.from_numpy(at), T)
    assert pos.dtype == torch.int64 and sorted(pos.tolist()) == list(range(len(want)))
    moved = torch.empty_like(got).index_copy_(0, pos, got) if len(want) else got
    assert np.array_equal(moved.numpy(), np.sort(want))


def test_row_map_beyond_int32():
    from lidar4d_amd import cull
    T = 768
    live = torch.tensor([2 ** 22 + 5], dtype=torch.int32)  # r * T = 3.2e9: the map is int64 arithmetic
    got = cull.slab_map(live, T, 704, 64)
    assert got[0].item() == (2 ** 22 + 5) * T + 704 and got[-1].item() == (2 ** 22 + 5) * T + 767


# ---- Trainer -----------------------------------------------------------------------------------------------------------------------
def test_trainer_with_cull_is_not_captured():
    from lidar4d_amd.trainer import Trainer
    sig = inspect.signature(Trainer.__init__)
    assert sig.parameters["cull"].default is None and sig.parameters["cull_slab"].default == 128
    tr = Trainer.__new__(Trainer)
    tr.model = types.SimpleNamespace(fused=True, _store=types.SimpleNamespace(flat=types.SimpleNamespace(is_cuda=True)))
    tr.dataset = types.SimpleNamespace(batch_for=None, next_frame=None)
    tr.reducer, tr.urf = None, False
    assert tr.graphs_supported() is True  # (a bare trainer on a device-resident model and dataset: nothing needs the host)
    tr.cull, tr.cull_slab = None, 128
    assert tr.graphs_supported() is True
    for eps in (1e-4, 0.0):
        tr.cull = eps
        assert tr.graphs_supported() is False
        with pytest.raises(RuntimeError, match="graphs_supported"):
            tr.train_step_graphed()


def test_trainer_hands_cull_to_render():
    """``_step_device_work`` renders with ``cull`` / ``slab`` when set, and with neither keyword when not."""
    from lidar4d_amd.trainer import Trainer
    seen = []

    class Stop(Exception):
        pass

    class Model:
        _store = types.SimpleNamespace(flat=torch.zeros(1))

        def render(self, rays_o, rays_d, time, **kw):
            seen.append(kw)
            raise Stop

    data = {"rays_o_lidar": torch.zeros(1, 8, 3), "rays_d_lidar": torch.zeros(1, 8, 3), "time": torch.zeros(1, 1)}
    for kw, want in (({}, (None, None)), ({"cull": 1e-4, "cull_slab": 64}, (1e-4, 64)), ({"cull": 0.0, "cull_slab": 128}, (0.0, 128))):
        tr = Trainer.__new__(Trainer)
        tr.model, tr.num_steps, tr.flow = Model(), 32, False
        tr.opt = types.SimpleNamespace(zero_grad=lambda: None)
        for k, v in kw.items():
            setattr(tr, k, v)
        with pytest.raises(Stop):
            tr._step_device_work(data)
        got = seen.pop()
        assert (got.get("cull"), got.get("slab")) == want and got["perturb"] is True and got["staged"] is False
        assert ("cull" in got) == bool(kw)
