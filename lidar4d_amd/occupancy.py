"""Empty-space skipping for no-grad renders: ``LiDAR4D.render(..., early_stop=eps, slab=S, occupancy=grid)``.

``early_stop`` stops evaluating a ray BEHIND its first opaque surface; an ``OccupancyGrid`` lets the same march skip the empty air IN
FRONT of it.  The grid is R^3 bits over the scene box.  ``l4d_sample_rays`` (ABI 6) tests every sample of a ray against it and
returns one flag per (ray, slab): does any sample of that slab lie in a set cell.  The march (early_stop.py) then evaluates a slab's
rows only for the rays that are alive AND flagged in it.

Semantics, exactly: the result is the full render with sigma set to 0 at every sample of a skipped (ray, slab) and behind each ray's
retirement point.  A skipped slab leaves the ray's transmittance as it is (its factors (1 - 0) + 1e-15f are exactly 1.0f); the
outputs come from the plain render's own stages on that dense sigma.  ``early_stop=0.0`` skips without ever retiring.

The grid that ``OccupancyGrid.build`` makes is a HEURISTIC, not a conservative bound: a cell is set when the largest density found
at a few probe points in it gives a per-sample optical depth of at least ``min_depth``, and the set is dilated.  A thin structure
between the probes can be missed, and ``min_depth = 1e-3`` is a starting value nobody has measured.  ``OccupancyGrid.audit`` is the tool
to check a grid on one's own scene: it returns, per ray, what the skipped samples hold in the full render and the bound that follows.

Training through the grid is not built (``cull`` is unchanged); there is no library of its own: the probes go through the entry
points the march uses per slab, and packing the bits is plain torch arithmetic, once per frame.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import ops


def _time_value(time):
    """The one time of a frame as a python float (fp32-rounded)."""
    if torch.is_tensor(time):
        if time.numel() != 1:
            raise ValueError(f"occupancy: one grid holds one frame's time, got a time tensor of {time.numel()} elements")
        return float(time.reshape(-1)[0].float())
    return float(np.float32(time))


def _check_model(model):
    if not getattr(model, "fused", False):
        raise ValueError("occupancy needs the fused pipeline (model.fused): this model renders through density() / attribute(), "
                         "which evaluate every sample")
    if torch.is_grad_enabled() and hasattr(model, "_store") and any(p.requires_grad for _, p, _, n, _ in model._store.entries if n > 0):
        raise ValueError("occupancy renders without a gradient: a field parameter requires grad and grad mode is on "
                         "(wrap the call in torch.no_grad(); training through the grid is not supported)")


def field_sigma(model, xt, t_dev, tinfo, rows_like_points=None):
    """sigma [P] fp32 and h [P, 16] fp16 of the rows xt [P, 4] = (x, y, z in [0, 1], t): the calls ``early_stop.run`` makes per slab --
    flow grid, flow network, field encode, density network -- with nothing kept for a backward."""
    from .fused import _field_desc, _flow_w16
    store, fn, sn = model._store, model.flow_net, model.sigma_net
    xf = ops.hashgrid_t_fwd(fn.grid_enc.meta, xt, (0, 1, 2), [store.half(fn.grid_enc.params)], t_dev, half_out=True)
    flow16, _ = ops.mlp_fwd(xf, _flow_w16(model), fn.n_hidden, hidden=fn.hidden_dim, save_act=False)
    if sn.n_neurons == 64:
        _, h, _, sigma = ops.density_encode_fwd(_field_desc(model), xt, flow16, tinfo, sn.in_pad, sigma_weights16=store.half(sn.params),
                                                n_hidden=sn.n_hidden_layers, save_act=False, rows_like_points=rows_like_points)
    else:
        X = ops.density_encode_fwd(_field_desc(model), xt, flow16, tinfo, sn.in_pad, rows_like_points=rows_like_points)
        h, _, sigma = ops.mlp_fwd_sigma(X, store.half(sn.params), sn.n_hidden_layers, save_act=False, hidden=sn.n_neurons)
    return sigma, h


def pack_bits(mask):
    """bool [R, R, R] indexed [z, y, x] -> int32 [ceil(R^3 / 32)]: cell i = (z R + y) R + x is bit i & 31 of word i >> 5."""
    flat = mask.reshape(-1).to(torch.int64)
    pad = (-flat.numel()) % 32
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    words = (flat.view(-1, 32) << torch.arange(32, dtype=torch.int64, device=flat.device)).sum(1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


def for_frame(model, time, num_steps, occupancy):
    """The render keywords of a caller's ``occupancy`` option: none for None; else the grid of this frame -- built here from a dict of
    ``OccupancyGrid.build``'s keywords, at the frame's time and from the weights the model holds now -- as ``occupancy=``."""
    if occupancy is None:
        return {}
    if not isinstance(occupancy, dict):
        raise ValueError(f"occupancy must be None or a dict of OccupancyGrid.build's keywords, got {occupancy!r}")
    return {"occupancy": OccupancyGrid.build(model, time, num_steps=num_steps, **occupancy)}


class OccupancyGrid:
    """R^3 occupancy bits over the scene box [-bound, bound]^3, on the model's device.  ``bits``: int32 words, cell (cx, cy, cz) at bit
    i & 31 of word i >> 5 with i = (cz R + cy) R + cx.  ``time``, ``num_steps``, ``min_depth``: what the grid was built for, or None
    (a grid from a mask holds for any); the march refuses a grid whose ``bound``, ``time`` or ``num_steps`` is not the call's."""

    def __init__(self, bits, R, bound, time=None, num_steps=None, min_depth=None):
        self.bits, self.R, self.bound = bits, int(R), bound
        self.time, self.num_steps, self.min_depth = time, num_steps, min_depth

    @classmethod
    def from_mask(cls, mask, bound, time=None):
        """mask: bool [R, R, R] indexed [z, y, x], any R >= 1."""
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.dim() != 3 or len(set(mask.shape)) != 1 or mask.shape[0] < 1:
            raise ValueError("OccupancyGrid.from_mask: mask must be a bool [R, R, R] tensor with R >= 1")
        return cls(pack_bits(mask), mask.shape[0], bound, time=None if time is None else _time_value(time))

    def mask(self):
        """-> bool [R, R, R] indexed [z, y, x]"""
        R = self.R
        bit = (self.bits.to(torch.int64).unsqueeze(1) >> torch.arange(32, dtype=torch.int64, device=self.bits.device)) & 1
        return bit.reshape(-1)[:R ** 3].view(R, R, R).bool()

    def check_call(self, model, time, num_steps):
        """Raises unless the grid is for this model's box, and, where it says, for this time and this number of samples."""
        if float(self.bound) != float(model.bound):
            raise ValueError(f"occupancy: the grid's bound {self.bound!r} is not the model's {model.bound!r}")
        if self.num_steps is not None and int(self.num_steps) != int(num_steps):
            raise ValueError(f"occupancy: the grid was built for num_steps={self.num_steps}, the call has {num_steps}")
        if self.time is not None and _time_value(time) != self.time:
            raise ValueError(f"occupancy: the grid was built for time {self.time!r}, the call has {_time_value(time)!r}")

    @staticmethod
    def probe_rows(cells, R, probes, a, t):
        """xt rows [n, 4] fp32 of probe a = (ax, ay, az) of the cells with flat indices ``cells`` (int64): coordinate d is
        (c_d + (a_d + 0.5) / probes) / R, in the normalised [0, 1]^3 coordinates of an xt row; column 3 is t."""
        c = torch.stack([cells % R, (cells // R) % R, cells // (R * R)], dim=1).to(torch.float32)
        off = torch.tensor([(k + 0.5) / probes for k in a], dtype=torch.float32, device=cells.device)
        xyz = (c + off) / float(R)
        return torch.cat([xyz, torch.full_like(xyz[:, :1], t)], dim=1).contiguous()

    @classmethod
    def build(cls, model, time, num_steps=768, resolution=128, probes=2, min_depth=1e-3, dilate=1, max_rows=1 << 21):
        """The grid of one frame from the field itself.  Every cell gets probes^3 probe points (``probe_rows``); a cell is occupied
        iff the largest sigma found there gives a per-sample optical depth max(sigma) * density_scale * sample_dist * (2 if
        active_sensor else 1) >= min_depth -- the product ``l4d_composite_fwd`` exponentiates, sample_dist = (far - near) / num_steps in
        fp32 -- and the set is dilated by ``dilate`` cells.  Rows are evaluated ``max_rows`` at a time.  No-grad, fused models only.

        ``min_depth = 1e-3`` is a starting value that nobody has measured on a trained scene, and the grid is a heuristic, not a
        conservative bound (the field between the probes is not seen): validate it with ``audit`` on your own scene."""
        _check_model(model)
        R, probes, dilate, max_rows = int(resolution), int(probes), int(dilate), int(max_rows)
        if R < 1 or probes < 1 or dilate < 0 or max_rows < 1:
            raise ValueError("OccupancyGrid.build: resolution, probes and max_rows must be at least 1 and dilate at least 0")
        dev = next(model.parameters()).device
        t = _time_value(time)
        near32, far32 = np.float32(model.near_lidar), np.float32(model.far_lidar)
        sample_dist = float(np.float32(far32 - near32) / np.float32(int(num_steps)))
        with torch.no_grad(), torch.autocast(device_type=dev.type, enabled=False):
            t_dev = torch.tensor([t], dtype=torch.float32, device=dev)
            tinfo = ops.time_setup(t_dev, model.num_frames)
            top = torch.zeros(R ** 3, dtype=torch.float32, device=dev)
            for c0 in range(0, R ** 3, max_rows):
                cells = torch.arange(c0, min(R ** 3, c0 + max_rows), dtype=torch.int64, device=dev)
                for az in range(probes):
                    for ay in range(probes):
                        for ax in range(probes):
                            sigma, _ = field_sigma(model, cls.probe_rows(cells, R, probes, (ax, ay, az), t), t_dev, tinfo)
                            top[c0:c0 + cells.numel()] = torch.maximum(top[c0:c0 + cells.numel()], sigma)
            depth = top * float(model.density_scale) * sample_dist * (2.0 if model.active_sensor else 1.0)  # (fp32, left to right)
            occupied = (depth >= float(min_depth)).view(1, 1, R, R, R)
            if dilate:
                occupied = F.max_pool3d(occupied.float(), 2 * dilate + 1, stride=1, padding=dilate) > 0
            return cls(pack_bits(occupied.view(R, R, R)), R, model.bound, time=t, num_steps=int(num_steps), min_depth=float(min_depth))

    def flags(self, model, rays_o, rays_d, num_steps, slab):
        """-> z_vals [N, T] and flags [N, ceil(T / slab)] uint8 of the un-jittered samples of the rays [N, 3] (``ops.sample_rays``)."""
        near32, far32 = np.float32(model.near_lidar), np.float32(model.far_lidar)
        z_vals, _, flags = ops.sample_rays(rays_o, rays_d, model._lin(int(num_steps), rays_o.device), None, float(near32), float(far32),
                                           model.bound, want_xyz=False, occ=(self.bits, self.R), slab=slab)
        return z_vals, flags

    def audit(self, model, rays_o, rays_d, time, num_steps, slab):
        """What this grid would skip on these rays, measured on the FULL no-grad render (no early_stop, no occupancy: every sample
        evaluated once, the plain render's density stage and ``composite_fwd``) plus one flags call.  rays [..., 3].  -> dict of

          D [N] float64              the sum, over the samples of the ray's skipped slabs, of the full render's per-sample optical
                                     depth tau_s = delta_s * density_scale * sigma_s * (2 if active_sensor else 1)
          skipped_weight [N] float64 the full render's weight on those samples
          flags [N, n_slabs] uint8, weights [N, T], weights_sum [N], depth [N], z_vals [N, T]: the flags and the full render

        What follows from D for ``render(..., early_stop=0.0, slab=slab, occupancy=self)`` against the full render, up to the 1e-15
        term of the transmittance factors and fp32 rounding: skipping multiplies the transmittance in front of sample s by
        e^{D_s}, D_s <= D the skipped optical depth in front of s, so

          every evaluated sample's weight w' lies in [w, w e^D];
          the weight lost on the skipped samples is at most 1 - e^{-D};
          hence |d weights_sum| <= e^D - 1 + D  and  |d depth| <= far_lidar (e^D - 1 + D).

        What fp32 rounding means here: a transmittance factor is formed to about 2^-24 absolute (for tau above 17 it is 1e-15
        whatever tau is), so the full render's weights carry an absolute error of up to about 2 T 2^-24, and skipping multiplies that
        error by e^D like the weight itself: the first line reads w' <= (w + 2 T 2^-24) e^D, and it says something while e^D is
        far below 2^24 / T.  A grid is good for a scene when D is small on its rays; a ray with a large D crosses density that
        the grid calls empty (raise ``probes`` or ``dilate``, or lower ``min_depth``)."""
        _check_model(model)
        self.check_call(model, time, num_steps)
        T = int(num_steps)
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N, dev = rays_o.shape[0], rays_o.device
        near32, far32 = np.float32(model.near_lidar), np.float32(model.far_lidar)
        sample_dist = float(np.float32(far32 - near32) / np.float32(T))
        with torch.no_grad(), torch.autocast(device_type=dev.type, enabled=False):
            t_dev = torch.tensor([_time_value(time)], dtype=torch.float32, device=dev)
            tinfo = ops.time_setup(t_dev, model.num_frames)
            lin = model._lin(T, dev)
            z_vals, xt = ops.sample_rays_xt(rays_o, rays_d, lin, None, t_dev, float(near32), float(far32), model.bound)
            sigma, _ = field_sigma(model, xt, t_dev, tinfo)
            sigma = sigma.view(N, T)
            weights, wsum, depth, _, _, _ = ops.composite_fwd(sigma, z_vals, sample_dist, model.density_scale, model.active_sensor,
                                                              want_mask=False, want_idx=False)
            _, flags = self.flags(model, rays_o, rays_d, T, slab)
            skipped = ~flags.bool().repeat_interleave(int(slab), dim=1)[:, :T]
            D, lost = skipped_depth(sigma, z_vals, weights, skipped, sample_dist, model.density_scale, model.active_sensor)
        return {"D": D, "skipped_weight": lost, "flags": flags, "weights": weights, "weights_sum": wsum, "depth": depth, "z_vals": z_vals}


def skipped_depth(sigma, z_vals, weights, skipped, sample_dist, density_scale, active_sensor):
    """-> D [N], lost [N] float64: the optical depth and the weight of a render's samples marked in ``skipped`` (bool [N, T])."""
    z = z_vals.double()
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], float(sample_dist))], dim=1)
    tau = delta * float(density_scale) * sigma.double() * (2.0 if active_sensor else 1.0)
    zero = torch.zeros((), dtype=torch.float64, device=tau.device)
    return torch.where(skipped, tau, zero).sum(1), torch.where(skipped, weights.double(), zero).sum(1)
