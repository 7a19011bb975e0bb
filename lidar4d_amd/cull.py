"""Training on culled samples: ``LiDAR4D.run(..., cull=eps, slab=S)`` with grad mode on and field parameters that require grad.

``early_stop.py``'s march inside the training step.  The samples and their jitter are the plain training render's: ``z_vals`` is
``RenderFn``'s, bit for bit, for the same ``noise``.  A ray's samples are evaluated front to back in slabs of ``S``; after each slab
``l4dr_slab_update`` -- as it stands, on the jittered ``z_vals`` -- forms the ray's transmittance so far and retires the ray once it is
below ``eps`` (``early_stop.py`` has the rule).  ``retired_at[r]`` is the number of samples of ray r that were evaluated, a multiple of
S or T; ``evaluated_samples`` is their sum.

The result is, by definition, the plain training render with sigma replaced by ``sigma * M``, ``M[r, s] = (s < retired_at[r])`` taken as
a CONSTANT.  The compositing, the attribute networks (``attribute_stage(..., train=True)``) and the image are the plain ones on the
dense sigma and h that ``l4dr_slab_update`` fills, so ``early_stop.py``'s bound carries over word for word:

  culled weights sum to T_s - T_end <= T_s < eps' = eps (1 + 1e-3)
  |d weights_sum| <= eps',  |d depth| <= eps' * far_lidar,  every culled weight < eps'
  weights, mask entries and attribute values at evaluated samples: unchanged
  eps <= 5e-5: no culled sample is in the full render's mask -> image_lidar and the mask list are identical; else |d image| <= eps'
  eps = 0: no ray is ever retired

The backward is the exact adjoint of that masked function: culled samples receive no gradient and contribute none, and a parameter
touched only by culled samples keeps a zero gradient.  WHAT IS DROPPED against the plain backward is the adjoint of the samples behind a
retirement point, whose transmittance is below eps'.  Their sigma enters the outputs only through weights that sum to less than eps'
per ray, so each dropped d output / d sigma_k carries a factor T_k < eps'; but the dropped PARAMETER gradient is that times
d sigma_k / d theta, summed over up to T - S samples per ray, and sigma = exp(h0) behind a surface is not bounded by anything the march
knows.  The dropped part is NOT BOUNDED HERE.  (``M`` also depends on the parameters; as a step function of them it has derivative
zero almost everywhere, and none is taken.)

One pass, no second forward.  Per slab the forward keeps what the backward needs for the compact rows -- xt, xf, flow16, X, h, sigma
-- in buffers allocated once at their worst-case size (N * T rows: what the plain path keeps) and written at a running row offset
(``ops.sample_rays_xt(live=..., out=)``, ``ops.hashgrid_t_fwd(out=)``, ``ops.mlp_fwd(y=)``, ``ops.density_encode_fwd(X=, y=,
sigma=)``).  Hidden activations are kept only where ``ops.mlp_recompute_supported`` says the backward cannot recompute them; their
layout [layers, rows, width] cannot be addressed by a row offset, so there the slabs' pieces are concatenated along the rows after the
march.  Rows are slab-major: slab 0 of all rays, then slab 1 of the survivors, and so on; ``row_map`` keeps the dense flat index
``r * T + s`` of every compact row.  The backward runs ``composite_bwd`` and the attribute networks' backward dense, exactly as
``RenderFn.backward`` (``fused.composite_attribute_bwd``), gathers dh through the row map (torch indexing: plumbing) and runs the density
network's backward, the field encode's adjoint and the flow network's and grid's backward once over all P_c compact rows
(``fused.density_flow_bwd``).

The backward's rows are RAY-MAJOR: ray 0's evaluated samples, then ray 1's, the plain backward's order with the culled rows left out.
The hex-planes' adjoint (csrc/field_bwd.hip) sums the consecutive rows of a wavefront that fall into one cell in float and rounds
each such run once to its fixed point, so its result depends on which rows sit next to each other: on slab-major rows it differed from
the plain backward's by 1e-5 relative at eps = 0 (37 rays x 128 samples), a hundred times the distance between two plain passes.  So
the saved rows are moved once from their slab-major place i to ``ray_major_position`` = (evaluated samples of the rays in front) + s --
an exclusive sum over ``retired_at`` and one indexed copy per buffer, torch plumbing, no sort and no read-back -- and at eps = 0 the
backward sees exactly the plain rows in the plain order.  The encode adjoint's wave-level band skip needs every 64-row segment to be
consecutive samples of one ray; ray-major rows of rays that end at multiples of S have that when S % 64 == 0 and T % 64 == 0
(``samples_per_ray=64``, else 0).

THE HOST READS ONE int32 PER SLAB, the number of live rays, as the inference march does; nothing else is read back, and a culled step
is never captured into a graph (``Trainer.graphs_supported()`` is False while ``cull`` is set).
"""
import math

import numpy as np
import torch

from . import ops
from .fused import _field_desc, _flow_w16, attribute_stage, composite_attribute_bwd, density_flow_bwd


def check_options(model, cull, slab, early_stop, train):
    """What ``cull`` needs, checked before anything touches a device (``staged=True`` is refused by ``render``).  -> (eps, S)."""
    if isinstance(cull, bool) or not isinstance(cull, (int, float)) or not float(cull) >= 0.0 or math.isinf(cull):
        raise ValueError(f"cull must be None or a finite float >= 0 (the transmittance below which a ray is retired), got {cull!r}")
    if isinstance(slab, bool) or not isinstance(slab, int) or slab < 1:
        raise ValueError(f"slab must be a positive int (samples evaluated between two retirement tests), got {slab!r}")
    if early_stop is not None:
        raise ValueError("cull and early_stop are two forms of one march and cannot be given together: cull trains on the culled "
                         "samples, early_stop renders without a gradient")
    if not getattr(model, "fused", False):
        raise ValueError("cull needs the fused pipeline (model.fused): this model renders through density() / attribute(), "
                         "which evaluate every sample")
    if not train:
        raise ValueError("cull trains on culled samples and needs a gradient: grad mode is off or no field parameter requires grad "
                         "(for a render without a gradient use early_stop=..., which culls the same samples)")
    return float(cull), int(slab)


# ---- the row map ---------------------------------------------------------------------------------------------------------------
def slab_map(live, T, s0, Sp):
    """live: the rays (1-D integer tensor) of a slab of samples s0 .. s0 + Sp - 1.  -> [len(live) * Sp] int64, the dense flat index
    ``r * T + s`` of the slab's compact rows (ray-major inside the slab)."""
    s = torch.arange(s0, s0 + Sp, dtype=torch.int64, device=live.device)
    return (live.to(torch.int64).unsqueeze(1) * T + s.unsqueeze(0)).reshape(-1)


def row_map(live_lists, T, S):
    """live_lists[k]: the rays that are live in front of slab k (samples k * S .. min((k + 1) * S, T) - 1), one list per slab that
    runs.  -> int64 map from compact row (slab-major) to dense flat index."""
    pieces = [slab_map(live, T, k * S, min(S, T - k * S)) for k, live in enumerate(live_lists)]
    if not pieces:
        return torch.empty(0, dtype=torch.int64)
    return torch.cat(pieces)


def ray_major_position(rows, retired_at, T):
    """rows: the dense flat index ``r * T + s`` of every compact row (any order); retired_at [N]: samples evaluated per ray.  -> int64,
    the place of each row when the evaluated samples are laid out ray after ray: (evaluated samples of rays 0 .. r - 1) + s."""
    at = retired_at.to(torch.int64)
    first = torch.cumsum(at, 0) - at
    r = torch.div(rows, T, rounding_mode="floor")
    return first[r] + (rows - r * T)


# ---- the node --------------------------------------------------------------------------------------------------------------------
class CullFn(torch.autograd.Function):
    """``RenderFn`` with the density stage marched slab by slab on the live rays (forward) and differentiated on the compact rows it
    evaluated (backward).  Precisions and autocast handling are ``RenderFn``'s."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, model, rays_o, rays_d, t_dev, noise, num_steps, eps, S, *params):
        from . import early_stop as es
        store = model._store
        N, T = rays_o.shape[0], int(num_steps)
        P = N * T
        dev = rays_o.device
        near32, far32 = np.float32(model.near_lidar), np.float32(model.far_lidar)
        sample_dist = float(np.float32(far32 - near32) / np.float32(T))
        near, far = float(near32), float(far32)
        lin = model._lin(T, dev)
        tinfo = ops.time_setup(t_dev, model.num_frames)
        z_vals, _ = ops.sample_rays(rays_o, rays_d, lin, noise, near, far, model.bound, want_xyz=False)

        fn, sn = model.flow_net, model.sigma_net
        fd = _field_desc(model)
        keep_f = not ops.mlp_recompute_supported(fn.grid_enc.meta.n_levels * fn.grid_enc.meta.n_features // 4, fn.n_hidden, fn.hidden_dim)
        keep_s = sn.n_neurons != 64 or not ops.mlp_recompute_supported(sn.in_pad, sn.n_hidden_layers)
        # what the backward reads, compact and slab-major, at the worst case of N * T rows
        xt = torch.empty(P, 4, dtype=torch.float32, device=dev)
        xf = torch.empty(P, fn.grid_enc.meta.n_levels * fn.grid_enc.meta.n_features // 4, dtype=torch.float16, device=dev)
        flow16 = torch.empty(P, 16, dtype=torch.float16, device=dev)
        X = torch.empty(P, sn.in_pad, dtype=torch.float16, device=dev)
        h_c = torch.empty(P, 16, dtype=torch.float16, device=dev)
        sigma_c = torch.empty(P, dtype=torch.float32, device=dev)
        rows = torch.empty(P, dtype=torch.int64, device=dev)
        acts_f, acts_s = [], []
        # the dense arrays l4dr_slab_update fills for the plain compositing and attribute stage
        sigma = torch.empty(N, T, dtype=torch.float32, device=dev)
        h = torch.empty(P, 16, dtype=torch.float16, device=dev)
        retired_at = torch.empty(N, dtype=torch.int32, device=dev)
        trans, live, n_next = es.march_init(N, dev)
        live_next = torch.empty_like(live)
        n_live, s0, off = N, 0, 0
        while s0 < T and n_live > 0:
            Sp = min(S, T - s0)
            n = n_live * Sp
            sl = slice(off, off + n)
            rows[sl] = slab_map(live[:n_live], T, s0, Sp)
            # RenderFn.forward's calls on the slab's rows; the time planes in the form the whole batch takes (early_stop.run)
            ops.sample_rays_xt(rays_o, rays_d, lin, noise, t_dev, near, far, model.bound, live=live, n_live=n_live, s0=s0, S=S, out=xt[sl])
            ops.hashgrid_t_fwd(fn.grid_enc.meta, xt[sl], (0, 1, 2), [store.half(fn.grid_enc.params)], t_dev, out=xf[sl])
            _, a_f = ops.mlp_fwd(xf[sl], _flow_w16(model), fn.n_hidden, hidden=fn.hidden_dim, save_act=keep_f, y=flow16[sl])
            if sn.n_neurons == 64:
                _, _, a_s, _ = ops.density_encode_fwd(fd, xt[sl], flow16[sl], tinfo, sn.in_pad, X=X[sl], sigma_weights16=store.half(sn.params),
                                                      n_hidden=sn.n_hidden_layers, save_act=keep_s, rows_like_points=P, y=h_c[sl],
                                                      sigma=sigma_c[sl])
            else:
                ops.density_encode_fwd(fd, xt[sl], flow16[sl], tinfo, sn.in_pad, X=X[sl], rows_like_points=P)
                _, a_s, _ = ops.mlp_fwd_sigma(X[sl], store.half(sn.params), sn.n_hidden_layers, save_act=True, hidden=sn.n_neurons,
                                              y=h_c[sl], sigma=sigma_c[sl])
            if a_f is not None:
                acts_f.append(a_f)
            if a_s is not None:
                acts_s.append(a_s)
            es.slab_update(sigma_c[sl], h_c[sl], z_vals, live, n_live, s0, S, sample_dist, model.density_scale, model.active_sensor, eps,
                           trans, sigma, h, retired_at, live_next, n_next)
            off += n
            s0 += Sp
            live, live_next = live_next, live
            if s0 < T:
                n_live = int(n_next.item())  # THE read-back: four bytes per slab, the size of the next slab's launches
        # (activations: [layers, rows, width] per slab -> one array over all compact rows; only shapes the backward cannot recompute)
        act_f = torch.cat(acts_f, dim=1) if acts_f else None
        act_s = torch.cat(acts_s, dim=1) if acts_s else None

        weights, wsum, depth, _, idx, count = ops.composite_fwd(sigma, z_vals, sample_dist, model.density_scale, model.active_sensor,
                                                                want_mask=False, want_idx=True)
        image, gathered, XA, actR, actI, attr, attr_c, denc = attribute_stage(model, rays_d, h, weights, idx, count, T, True)
        evaluated = torch.tensor(off, dtype=torch.int64, device=dev)

        ctx.model, ctx.T, ctx.sample_dist, ctx.gathered, ctx.n_rows = model, T, sample_dist, gathered, off
        ctx.samples_per_ray = 64 if S % 64 == 0 and T % 64 == 0 else 0
        ctx.slice_pair = getattr(model, "_host_slice_pair", None)
        ctx.save_for_backward(t_dev, tinfo, z_vals, xt, xf, flow16, act_f, X, h, act_s, sigma, weights, idx, count, XA, actR, actI,
                              attr, attr_c, denc, rows, retired_at)
        ctx.mark_non_differentiable(z_vals, idx, count, evaluated, retired_at)
        return depth, image, wsum, weights, z_vals, idx, count, evaluated, retired_at

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_depth, d_image, d_wsum, d_weights, _dz, _di, _dc, _de, _dr):
        model, T, Pc = ctx.model, ctx.T, ctx.n_rows
        (t_dev, tinfo, z_vals, xt, xf, flow16, act_f, X, h, act_s, sigma, weights, idx, count, XA, actR, actI, attr, attr_c, denc,
         rows, retired_at) = ctx.saved_tensors
        dh = composite_attribute_bwd(model, T, ctx.sample_dist, ctx.gathered, tinfo, z_vals, h, sigma, weights, idx, count, XA, actR, actI,
                                     attr, attr_c, denc, d_depth, d_wsum, d_image, d_weights)
        # slab-major -> ray-major (the module's docstring says why): every saved buffer once, dh straight from its dense rows
        rows = rows[:Pc]
        pos = ray_major_position(rows, retired_at, T)
        # (indexed copies: as gathers through the inverse map the moves measured 7 ms slower at 12.6 M rows)
        move = lambda a, dim=0: None if a is None else torch.empty_like(a.narrow(dim, 0, Pc)).index_copy_(dim, pos, a.narrow(dim, 0, Pc))
        dh_c = dh.index_select(0, move(rows))  # the adjoint rows of the evaluated samples; the culled rows' stay behind
        density_flow_bwd(model, t_dev, tinfo, move(xt), move(xf), move(flow16), move(act_f, 1), move(X), move(act_s, 1), dh_c,
                         ctx.samples_per_ray, ctx.slice_pair)
        return (None,) * 8 + (None,) * (len(ctx.needs_input_grad) - 8)


def run(model, rays_o, rays_d, t_dev, noise, num_steps, eps, S, params):
    """-> depth, image, wsum, weights, z_vals, idx, count (as RenderFn), evaluated_samples (int64 scalar), retired_at [N] int32."""
    return CullFn.apply(model, rays_o, rays_d, t_dev, noise, num_steps, eps, S, *params)
