"""Early ray termination for no-grad renders: ``LiDAR4D.run(..., early_stop=eps, slab=S)``.

A LiDAR ray ends at the first opaque surface; every sample behind it has a weight below the ``1e-4`` mask threshold and still costs
the flow grid, the flow network, the field encode and the density network.  Here a ray's samples are evaluated front to back in slabs
of ``S``; after each slab the ray's transmittance so far, T^ = prod((1 - alpha_k) + 1e-15) with ``composite_fwd``'s alpha, is formed on
the device, and a ray with T^ < eps is retired: its remaining samples are not evaluated and count as sigma = 0.  The outputs then
come from the plain render's own stages -- ``ops.composite_fwd``, the attribute networks on its work list, ``ops.composite_image`` -- on
the dense sigma, so the result is exactly "the full render with sigma zeroed behind each ray's retirement point":

  culled weights sum to T_s - T_end <= T_s < eps' = eps (1 + 1e-3)   (T^ is T_s to within 2 T 2^-24 relative)
  |d weights_sum| <= eps',  |d depth| <= eps' * far_lidar,  every culled weight < eps'
  weights, mask entries and attribute values at evaluated samples: unchanged (prefix products do not see later samples)
  eps <= 5e-5: no culled sample is in the full render's mask -> image_lidar and the mask list are identical; else |d image| <= eps'
  eps = 0: no ray is ever retired

(tests/early_stop_ref.py has the derivation.  "Unchanged" means the plain render's bits where the field encode takes the same form on
a slab's rows as on the whole batch -- see the comment in ``run`` -- and the encode's own rounding between its forms otherwise.)  Per slab the field kernels run on compact rows of the live rays only
(include/lidar4d_march.h: l4dr_slab_rows in front, l4dr_slab_update behind), and the HOST READS ONE int32, the number of live
rays, to size the next slab's launches: a deliberate exception to "no host synchronisation", for inference only.  Nothing else is
read back, and a march is never captured into a graph.

With ``occupancy=grid`` (occupancy.py) the march also skips empty space in FRONT of the surface: a slab of a ray is evaluated only
where the ray is alive and one of the slab's samples lies in a set cell of the grid (``run_skipping``).  The result is then the full
render with sigma set to 0 at every sample of a skipped (ray, slab) and behind each ray's retirement point; what that costs in
accuracy depends on the grid and is what ``OccupancyGrid.audit`` measures.
"""
import math

import numpy as np
import torch

from . import ops
from .fused import _field_desc, _flow_w16, attribute_stage
from .ops import _chk, _p, _stream


def _call(name, *args):
    from . import _march_lib  # liblidar4d_march.so: mapped on first use
    _march_lib.call(name, *args)


def check_options(model, early_stop, slab, perturb, train):
    """What ``early_stop`` needs, checked before anything touches a device.  -> (eps, S)."""
    if isinstance(early_stop, bool) or not isinstance(early_stop, (int, float)) or not float(early_stop) >= 0.0 or math.isinf(early_stop):
        raise ValueError(f"early_stop must be None or a finite float >= 0 (the transmittance below which a ray is retired), got {early_stop!r}")
    if isinstance(slab, bool) or not isinstance(slab, int) or slab < 1:
        raise ValueError(f"slab must be a positive int (samples evaluated between two retirement tests), got {slab!r}")
    if not getattr(model, "fused", False):
        raise ValueError("early_stop needs the fused pipeline (model.fused): this model renders through density() / attribute(), "
                         "which evaluate every sample")
    if perturb:
        raise ValueError("early_stop is for inference: perturb=True (jittered samples) is a training option and is not supported with it")
    if train:
        raise ValueError("early_stop renders without a gradient: a field parameter requires grad and grad mode is on "
                         "(wrap the call in torch.no_grad(); training on culled samples is not supported)")
    return float(early_stop), int(slab)


# ---- the two entry points ---------------------------------------------------------------------------------------------------
def march_init(N, device):
    """-> trans [N] fp32 = 1, live [N] int32 = 0 .. N - 1, n_live [1] int32 = N"""
    trans = torch.empty(N, dtype=torch.float32, device=device)
    live = torch.empty(N, dtype=torch.int32, device=device)
    n_live = torch.empty(1, dtype=torch.int32, device=device)
    _chk(trans, torch.float32, "trans")
    _call("l4dr_march_init", N, _p(trans), _p(live), _p(n_live), _stream())
    return trans, live, n_live


def slab_rows(rays_o, rays_d, lin, t_dev, live, n_live, s0, S, near, far, bound):
    """-> xt [n_live * S', 4] fp32: ``ops.sample_rays_xt``'s rows (no noise) of samples s0 .. s0 + S' - 1 of the rays live[:n_live]."""
    _chk(rays_o, torch.float32, "rays_o"), _chk(rays_d, torch.float32, "rays_d"), _chk(lin, torch.float32, "lin")
    _chk(t_dev, torch.float32, "t"), _chk(live, torch.int32, "live")
    N, T = rays_o.shape[0], lin.shape[0]
    if n_live > live.numel():
        raise ValueError("slab_rows: n_live exceeds the live list")
    Sp = max(0, min(S, T - s0))
    xt = torch.empty(n_live * Sp, 4, dtype=torch.float32, device=rays_o.device)
    _call("l4dr_slab_rows", _p(rays_o), _p(rays_d), _p(lin), _p(t_dev), _p(live), n_live, N, T, s0, S, float(near), float(far),
          float(bound), _p(xt), _stream())
    return xt


def slab_update(sigma_c, h_c, z_vals, live, n_live, s0, S, sample_dist, density_scale, active_sensor, eps, trans, sigma_dense,
                h_dense, retired_at, live_next, n_live_next):
    """See include/lidar4d_march.h.  Updates trans / sigma_dense / h_dense / retired_at in place; fills live_next, n_live_next."""
    _chk(sigma_c, torch.float32, "sigma_c"), _chk(h_c, torch.float16, "h_c"), _chk(z_vals, torch.float32, "z_vals")
    _chk(live, torch.int32, "live"), _chk(trans, torch.float32, "trans"), _chk(sigma_dense, torch.float32, "sigma_dense")
    _chk(h_dense, torch.float16, "h_dense"), _chk(retired_at, torch.int32, "retired_at"), _chk(live_next, torch.int32, "live_next")
    _chk(n_live_next, torch.int32, "n_live_next")
    N, T = z_vals.shape
    Sp = max(0, min(S, T - s0))
    if (n_live > live.numel() or n_live > live_next.numel() or sigma_c.numel() < n_live * Sp or h_c.numel() < n_live * Sp * 16
            or h_c.shape[-1] != 16 or h_dense.shape[-1] != 16 or sigma_dense.numel() != N * T or h_dense.numel() != N * T * 16
            or trans.numel() != N or retired_at.numel() != N):
        raise ValueError("slab_update: a buffer is smaller than n_live rays of this slab need")
    if live.data_ptr() == live_next.data_ptr():
        raise ValueError("slab_update: live_next must not be live")
    from . import _march_lib
    ws = torch.empty(_march_lib.lib().l4dr_slab_update_workspace(n_live), dtype=torch.uint8, device=z_vals.device)
    _call("l4dr_slab_update", _p(sigma_c), _p(h_c), _p(z_vals), _p(live), n_live, N, T, s0, S, float(sample_dist), float(density_scale),
          int(bool(active_sensor)), float(eps), _p(trans), _p(sigma_dense), _p(h_dense), _p(retired_at), _p(live_next), _p(n_live_next),
          _p(ws), _stream())


# ---- the march -----------------------------------------------------------------------------------------------------------------
def run(model, rays_o, rays_d, t_dev, num_steps, eps, S, occupancy=None):
    """``RenderFn.forward`` with the density stage walked slab by slab.  rays_o / rays_d [N, 3] fp32, t_dev one fp32 on the device.
    -> depth, image, wsum, weights, z_vals, idx, count (as RenderFn), evaluated_samples (int64 scalar), retired_at [N] int32.
    occupancy: an ``occupancy.OccupancyGrid`` -- the march of ``run_skipping`` below; None: this function as it always was."""
    if occupancy is not None:
        return run_skipping(model, rays_o, rays_d, t_dev, num_steps, eps, S, occupancy)
    store = model._store
    N, T = rays_o.shape[0], int(num_steps)
    dev = rays_o.device
    near32, far32 = np.float32(model.near_lidar), np.float32(model.far_lidar)
    sample_dist = float(np.float32(far32 - near32) / np.float32(T))
    with torch.no_grad(), torch.autocast(device_type=dev.type, enabled=False):
        lin = model._lin(T, dev)
        tinfo = ops.time_setup(t_dev, model.num_frames)
        z_vals, _ = ops.sample_rays(rays_o, rays_d, lin, None, float(near32), float(far32), model.bound, want_xyz=False)
        sigma = torch.empty(N, T, dtype=torch.float32, device=dev)
        h = torch.empty(N * T, 16, dtype=torch.float16, device=dev)
        retired_at = torch.empty(N, dtype=torch.int32, device=dev)
        trans, live, n_next = march_init(N, dev)
        live_next = torch.empty_like(live)
        fn, sn = model.flow_net, model.sigma_net
        fd = _field_desc(model)
        n_live, s0, evaluated = N, 0, 0
        while s0 < T and n_live > 0:
            Sp = min(S, T - s0)
            xt = slab_rows(rays_o, rays_d, lin, t_dev, live, n_live, s0, S, float(near32), float(far32), model.bound)
            # the calls of RenderFn.forward on the compact rows, nothing kept for a backward.  The time planes take the form the whole
            # batch would take (rows_like_points): with it a batch below ops.LDS_DYNHASH_MIN_POINTS samples gives the plain render's
            # bits at every evaluated sample.  Above, the encode's other forms (LDS-staged dynamic hash, level-major static grid,
            # density network as the kernel's epilogue) are chosen by the slab's own row count, as their workspaces are sized by it.
            xf = ops.hashgrid_t_fwd(fn.grid_enc.meta, xt, (0, 1, 2), [store.half(fn.grid_enc.params)], t_dev, half_out=True)
            flow16, _ = ops.mlp_fwd(xf, _flow_w16(model), fn.n_hidden, hidden=fn.hidden_dim, save_act=False)
            if sn.n_neurons == 64:
                _, h_c, _, sigma_c = ops.density_encode_fwd(fd, xt, flow16, tinfo, sn.in_pad, sigma_weights16=store.half(sn.params),
                                                            n_hidden=sn.n_hidden_layers, save_act=False, rows_like_points=N * T)
            else:
                X = ops.density_encode_fwd(fd, xt, flow16, tinfo, sn.in_pad, rows_like_points=N * T)
                h_c, _, sigma_c = ops.mlp_fwd_sigma(X, store.half(sn.params), sn.n_hidden_layers, save_act=False, hidden=sn.n_neurons)
            slab_update(sigma_c, h_c, z_vals, live, n_live, s0, S, sample_dist, model.density_scale, model.active_sensor, eps, trans,
                        sigma, h, retired_at, live_next, n_next)
            evaluated += n_live * Sp
            s0 += Sp
            live, live_next = live_next, live
            if s0 < T:
                n_live = int(n_next.item())  # THE read-back: four bytes per slab, the size of the next slab's launches
        weights, wsum, depth, _, idx, count = ops.composite_fwd(sigma, z_vals, sample_dist, model.density_scale, model.active_sensor,
                                                                want_mask=False, want_idx=True)
        image = attribute_stage(model, rays_d, h, weights, idx, count, T, False)[0]
        evaluated = torch.tensor(evaluated, dtype=torch.int64, device=dev)
    return depth, image, wsum, weights, z_vals, idx, count, evaluated, retired_at


def run_skipping(model, rays_o, rays_d, t_dev, num_steps, eps, S, grid):
    """``run`` with an occupancy grid (occupancy.py): a slab of a ray is evaluated only if the ray is alive AND some sample of that
    slab lies in a set cell of ``grid`` -- the flags ``l4d_sample_rays`` writes beside z_vals, one call up front.  The result is the
    full render with sigma set to 0 at every sample of a skipped (ray, slab) and behind each ray's retirement point: a skipped slab
    leaves the ray's transmittance as it is (its factors (1 - 0) + 1e-15f are exactly 1.0f), so ``trans`` stays composite_fwd's prefix
    product on that sigma.  Same returns as ``run``; ``retired_at`` is each ray's retirement point (T for a ray never retired) and
    ``evaluated_samples`` counts the rows actually evaluated.  The host reads one int32 per evaluated slab, as in ``run`` -- how many of the
    slab's rays go on -- and, only behind a slab that retired somebody, the number of rays with work in each slab ahead; a slab that every
    ray skips costs no read and no launch."""
    from .occupancy import field_sigma
    N, T = rays_o.shape[0], int(num_steps)
    dev = rays_o.device
    near32, far32 = np.float32(model.near_lidar), np.float32(model.far_lidar)
    sample_dist = float(np.float32(far32 - near32) / np.float32(T))
    with torch.no_grad(), torch.autocast(device_type=dev.type, enabled=False):
        lin = model._lin(T, dev)
        tinfo = ops.time_setup(t_dev, model.num_frames)
        z_vals, _, flags = ops.sample_rays(rays_o, rays_d, lin, None, float(near32), float(far32), model.bound, want_xyz=False,
                                           occ=(grid.bits, grid.R), slab=S)
        flags = flags.bool().t().contiguous()  # [n_slabs, N]
        sigma = torch.zeros(N, T, dtype=torch.float32, device=dev)
        h = torch.empty(N * T, 16, dtype=torch.float16, device=dev)  # (rows of samples never evaluated: sigma 0, weight 0, not listed)
        retired_at = torch.full((N,), T, dtype=torch.int32, device=dev)
        trans = torch.ones(N, dtype=torch.float32, device=dev)
        alive = torch.ones(N, dtype=torch.bool, device=dev)
        live_next, n_next = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        # work[k]: the rays alive now and flagged in slab k, on the host.  alive changes only when a slab retires somebody, so until
        # then the counts of the slabs ahead are exact: a slab nobody has work in costs nothing, and once no ray is alive the rest of
        # the walk is host arithmetic.
        work = flags.sum(1).tolist()
        s0, k, evaluated = 0, 0, 0
        while s0 < T:
            Sp = min(S, T - s0)
            n_act = work[k]
            if n_act > 0:
                active = torch.nonzero_static(alive & flags[k], size=n_act).view(-1).to(torch.int32)  # ascending, as ``run``'s live list
                xt = slab_rows(rays_o, rays_d, lin, t_dev, active, n_act, s0, S, float(near32), float(far32), model.bound)
                # (the calls of ``run`` on the compact rows, in the form the whole batch would take)
                sigma_c, h_c = field_sigma(model, xt, t_dev, tinfo, rows_like_points=N * T)
                slab_update(sigma_c, h_c, z_vals, active, n_act, s0, S, sample_dist, model.density_scale, model.active_sensor, eps, trans,
                            sigma, h, retired_at, live_next, n_next)
                evaluated += n_act * Sp
                # THE read-back, as in ``run``: how many of the slab's rays go on (eps = 0: nothing is ever retired, nothing is read).
                # If some do not, alive takes slab_update's own comparison on the same fp32 value and the counts are read again.
                if eps > 0 and s0 + Sp < T and int(n_next.item()) < n_act:
                    alive &= ~(trans < eps)
                    work = (flags & alive).sum(1).tolist()
            s0 += Sp
            k += 1
        weights, wsum, depth, _, idx, count = ops.composite_fwd(sigma, z_vals, sample_dist, model.density_scale, model.active_sensor,
                                                                want_mask=False, want_idx=True)
        image = attribute_stage(model, rays_d, h, weights, idx, count, T, False)[0]
        evaluated = torch.tensor(evaluated, dtype=torch.int64, device=dev)
    return depth, image, wsum, weights, z_vals, idx, count, evaluated, retired_at
