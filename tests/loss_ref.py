"""References and cases for the loss kernels' routes that the feature tests do not enter, shared by tests/test_loss_ref_cpu.py
(which pins the references) and tests/test_gpu_loss_edges.py (which holds the kernels to them).  Nothing here is computed by HIP
code: numpy, float64 where it says 64 and float32 in the kernel's operation order where it says emul.

Which case enters which route (the #defines are those of the .hip files named):

  kernel                               loop or branch                                              case
  -----------------------------------  ----------------------------------------------------------  ---------------------------------
  csrc/losses.hip  (LL_THREADS 256, LL_WAVES 4, LL_MAX_BLOCKS 2048; V = 4 where T % 4 == 0 and the pointers are 16-byte aligned)
  los_sums_kernel, los_grad_kernel     `t += 64 * V`, V = 4: second and third trip (T > 256)       40x768, 3x260_near_then_far,
                                                                                                   3x520_all_near
  los_sums_kernel, los_grad_kernel     `t += 64 * V`, V = 1: second and third trip (T > 64)        3x130_all_near
  los_pre_kernel                       chunk loop, first chunk all near, a later one not: m == 1   3x260_near_then_far
  los_pre_kernel                       chunk loop to the end, every sample near: m < 1, V = 4      3x520_all_near
  los_pre_kernel                       the same, V = 1                                             3x130_all_near
  all three                            `r += n_waves` (N > LL_MAX_BLOCKS * LL_WAVES = 8192)        8197x8, 8197x8_first_ray, 8197x6
  los_pre_kernel                       `one` set on a wave's SECOND ray decides m == 1             8197x8
  los_pre_kernel                       `one` set on ray 0, carried to ray 8192: `continue` after    8197x8_first_ray
                                       the hit count
  los_ray                              fp16 depth (bounds rounded to half) with V = 4              5x72_half_depth
  los_finish_kernel, los_grad_kernel   n_hit == 0: the IEEE result of the divisions                4x8_all_dropped
  l4dl_los_fwd / l4dl_los_bwd          T % 4 == 0 with a pointer that is not 16-byte aligned:      the C entry points on 40x768 and
                                       V = 1                                                       8197x8 inside larger buffers
  csrc/stepglue.hip
  step_criterion                       each of the four kinds for each of the three terms          all 64 triples (KINDS ** 3)
  step_criterion, L4DS_HUBER           |e| == delta, both signs, and a lattice step to either side  planted rows HUBER_ROWS
  step_criterion, L4DS_L1 / _HUBER     e == 0 for every term                                       planted row EXACT_ROW
  step_criterion, L4DS_BCE             expf(-a) = inf (a <= -89), expf(-|a|) = 0 (|a| >= 104)       planted rows LOGIT_ROWS
  step_primary_losses_kernel           the sigmoid in front of a BCE ray-drop term saturating       planted rows LOGIT_ROWS
  step_gt<true>                        products, clamp bounds rounded to half                      every triple with fp16 gt
  step_gt                              smooth = 0 (gs = m) and 0.5 (lo == hi)                      SETTINGS
  step_primary_losses_kernel           n at, one short of and one past a workgroup; n = 1          PRIMARY_N
  step_ray_batch_kernel                row outside [0, H): no pixel read, gt = 0                   tests/test_gpu_loss_edges.py
  step_ray_batch_kernel                `c < 0` after the C remainder of a negative column          tests/test_gpu_loss_edges.py
  csrc/patchgrad.hip  (PG_THREADS 256, PG_WAVES 4, PG_MAX_BLOCKS 1024)
  pg_sweep_kernel<false>               `group += gridDim.x` and the __syncthreads() between groups  patchgrad_cases 4101x8x8
  pg_sweep_kernel<true>                the same, BIG, pixel count no multiple of 256               patchgrad_cases 1030x5x13
  pg_sweep_kernel<false>               per_wave == 1 with idle lanes (33..64 pixels)               patchgrad_cases 9x5x7
  pg_scale_kernel                      `i += gridDim.x * PG_THREADS` (more than 262,144 elements)  patchgrad_cases 4101x8x8
  csrc/evalmeter.hip  (EM_THREADS 256, EM_CHUNK 2048, EM_MAX_BLOCKS 1024)
  eval_ssim_kernel, eval_finalize_..   `i += EM_THREADS` over more than 256 partials               meters_ref 8x65600
  eval_errors_kernel, eval_select_..   grid stride past EM_MAX_BLOCKS * EM_CHUNK = 2,097,152       meters_ref 8x262160 (+ _ties)
"""
import itertools

import numpy as np
import torch

import realdata_cases as rc
from test_gpu_los import _eps, _random_case  # (the ladder scheme is extended here, not changed)

F16, F32, F64 = np.float16, np.float32, np.float64
ITERS = 1000
STEPS = (0, 500, 2000)   # eps = 0.02, 0.00632, 0.002 (the last one is past iters: the exponent is clamped at 1)
MARGIN = 1e-5            # no sample of a case is closer than this to a bound at any of STEPS, the planted on-bound ones apart


# ==== line-of-sight loss ==================================================================================================================
def los_bounds(depth, eps):
    """-> (d, lo, hi) float32 [N] as csrc/losses.hip los_ray forms them: fp32 depths take ``d - eps32`` / ``d + eps32`` in float32;
    fp16 depths are widened, the sums taken in float32, rounded to half and widened again."""
    depth = np.asarray(depth)
    eps32 = F32(eps)
    d = depth.astype(F32)
    if depth.dtype == F16:
        return d, (d - eps32).astype(F16).astype(F32), (d + eps32).astype(F16).astype(F32)
    assert depth.dtype == F32
    return d, d - eps32, d + eps32


def _los_parts(z_vals, depth, step_or_count, iters, exact_two_var=False):
    """-> (near, empty, bell float64 [N,T], n_hit): the decisions the kernel's way, the bell in float64."""
    z = np.asarray(z_vals)
    assert z.dtype == F32 and z.ndim == 2
    eps = 0.02 * 0.1 ** min(step_or_count / iters, 1)  # float64, as python evaluates it
    d, lo, hi = los_bounds(np.asarray(depth).reshape(-1), eps)
    assert d.shape == (z.shape[0],)
    near = (z > lo[:, None]) & (z < hi[:, None])       # strict: a sample on a bound is neither near nor empty
    empty = (z < lo[:, None]) | (z > hi[:, None])
    two_var = 2 * (eps / 3) ** 2
    if not exact_two_var:
        two_var = float(F32(two_var))
    x = z.astype(F64) - d.astype(F64)[:, None]
    bell = np.where(near, np.exp(-(x * x) / two_var), 1.0)
    return near, empty, bell, int((d > 0).sum())


def los_ref64(weights, z_vals, depth, step_or_count, iters, upstream=1.0, m=None, exact_two_var=False):
    """The line-of-sight loss and d (upstream * loss) / d weights in float64 -> (loss, d_weights [N,T]).

    The decisions are taken the kernel's way: eps in float64 as python does, eps32 = float32(eps); bounds by ``los_bounds``; near
    and empty strict; two_var = float32(2 (eps / 3)^2).  Everything else is float64: x = z - d, bell = exp(-x x / two_var) at near
    samples and 1 elsewhere, m = max(bell), n_hit = count(d > 0), and per sample the term of los_grad_kernel -- w - bell / m where
    near, w where empty, 0 on a bound.  loss = 0.1 (sum(empty terms^2) / n_hit) + 0.1 (sum(near terms^2) / n_hit), the two
    quotients apart as the restatement and the kernel take them (with n_hit == 0 a sum of 0 gives NaN, any other inf);
    d_weights = upstream * 0.2 * term / n_hit.

    ``m``: a normaliser to use INSTEAD of max(bell) -- for the tests that show a wrong one is told apart.  ``exact_two_var``: divide
    by the float64 2 (eps / 3)^2 instead of its float32 rounding, which is what a float64 evaluation of ``urf_loss`` does; the two
    differ by up to 4.5 * 2^-24 relative in a bell value (the exponent is at most 4.5 inside the tolerance)."""
    w = np.asarray(weights)
    assert w.dtype == F32
    near, empty, bell, n_hit = _los_parts(z_vals, depth, step_or_count, iters, exact_two_var)
    assert w.shape == near.shape
    m = float(bell.max()) if m is None else float(m)
    w64 = w.astype(F64)
    term = np.where(near, w64 - bell / m, np.where(empty, w64, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        s_empty, s_near = F64((term * term)[empty].sum()), F64((term * term)[near].sum())
        loss = 0.1 * (s_empty / F64(n_hit)) + 0.1 * (s_near / F64(n_hit))
        d_weights = float(upstream) * 0.2 * term / F64(n_hit)
    return float(loss), d_weights


def los_bell_max(z_vals, depth, step, cols=None, iters=ITERS):
    """max(bell) over the columns ``cols`` (a slice; None: all) in float64 -- the normaliser a kernel would find that read those only."""
    near, empty, bell, _ = _los_parts(z_vals, depth, step, iters)
    return float(bell[:, cols if cols is not None else slice(None)].max())


def los_margin(z_vals, depth, step, skip=None):
    """The smallest distance of a sample from a bound at ``step`` (float64), the positions in the bool mask ``skip`` apart."""
    z = np.asarray(z_vals).astype(F64)
    d, lo, hi = los_bounds(np.asarray(depth).reshape(-1), _eps(step))
    dist = np.minimum(np.abs(z - lo.astype(F64)[:, None]), np.abs(z - hi.astype(F64)[:, None]))
    if skip is not None:
        dist = np.where(skip, np.inf, dist)
    return float(dist.min())


def _clear_of_bounds(z, d, skip=None):
    """Move every sample that is within 2 * MARGIN of a bound at one of STEPS by 1e-4, until none is (jittered ladders of 65,000
    samples hold a handful).  ``skip``: bool mask of samples that stay where they are (the ones planted ON a bound)."""
    z = z.clone()
    for _ in range(8):
        close = np.zeros(z.shape, dtype=bool)
        for step in STEPS:
            _, lo, hi = los_bounds(d.numpy(), _eps(step))
            zz = z.numpy().astype(F64)
            close |= np.minimum(np.abs(zz - lo.astype(F64)[:, None]), np.abs(zz - hi.astype(F64)[:, None])) < 2 * MARGIN
        if skip is not None:
            close &= ~skip
        if not close.any():
            return z
        z[torch.from_numpy(close)] += 1e-4
    raise AssertionError("samples stay close to a bound")


def _on_bounds_mask(N, T):
    skip = np.zeros((N, T), dtype=bool)
    if T >= 3:
        skip[0, T - 1] = skip[0, T - 2] = True
    return skip


def _ladder(N, T, seed, dropped=None, half=False, on_bounds=True):
    """test_gpu_los._random_case, cleared of samples that sit within 2e-5 of a bound by accident.  ``on_bounds=False`` moves the two
    samples it plants exactly on ray 0's bounds of step 0 three tenths of a millimetre outwards (for a float64 evaluation, whose
    bounds are not the float32 ones)."""
    w, z, d = _random_case(N, T, seed, dropped=dropped, half=half)
    skip = _on_bounds_mask(N, T)
    if not on_bounds and T >= 3:
        z[0, T - 1] -= 3e-4
        z[0, T - 2] += 3e-4
        skip = None
    return w, _clear_of_bounds(z, d, skip), d


NEAR_FAR_OFFSETS = (-0.015, -0.008, 0.009, 0.016, -0.012)  # all inside step 0's tolerance of 0.02, none closer than 8 mm
CLOSEST = 0.004                                            # bell = exp(-0.004^2 / (2 (0.02 / 3)^2)) = 0.835
FAR = (0.05, 0.1, -0.06, 0.2)


def _near_rows(T, closest_at=None, far_tail=False, seed=0):
    """[3, T]: depths 0.3, 0.5, 0.7 and samples at the depth + NEAR_FAR_OFFSETS repeated; ``closest_at``: that one column sits
    CLOSEST from the depth instead; ``far_tail``: the last four columns are FAR away."""
    d = torch.tensor([0.30, 0.50, 0.70])
    off = torch.tensor([NEAR_FAR_OFFSETS[t % len(NEAR_FAR_OFFSETS)] for t in range(T)])
    if closest_at is not None:
        off[closest_at] = CLOSEST
    if far_tail:
        off[T - 4:] = torch.tensor(FAR)
    z = (d[:, None] + off[None, :]).float()
    w = torch.rand(3, T, generator=torch.Generator().manual_seed(100 + seed)) * 0.9 + 0.05
    return w, z, d


RAY_OFFSETS = (-0.015, -0.008, CLOSEST, 0.009, 0.016, -0.012, 0.0011, -0.0045)  # all near at step 0; 0.0011 near at every step


def _many_rays(far_rays):
    """[8197, 8]: depths in (0.2, 0.8), every 97th ray dropped (depth 0), every sample at its ray's depth + RAY_OFFSETS -- all near
    at step 0, the dropped rays' too (around 0) -- except that the rays ``far_rays`` hold one sample 0.1 away.  Rays 0 and 8192 ..
    8196 have a return."""
    N, T = 8197, 8
    g = torch.Generator().manual_seed(31)
    d = 0.2 + 0.6 * torch.rand(N, generator=g)
    d[torch.arange(5, N, 97)] = 0.0
    assert float(d[0]) > 0 and bool((d[8192:] > 0).all())
    off = torch.tensor(RAY_OFFSETS).repeat(N, 1)
    off[:, 0] += (torch.rand(N, generator=g) - 0.5) * 0.002  # (-0.016 .. -0.014: the rays are not copies of each other)
    for r in far_rays:
        off[r, 5] = 0.1
    z = (d[:, None] + off).float()
    w = torch.rand(N, T, generator=g) * 0.9 + 0.05
    return w, _clear_of_bounds(z, d), d


def _all_dropped():
    """[4, 8], every depth 0 (n_hit == 0): a ladder over (0.05, 1) -- all empty -- with, on rays 1 and 3, samples within a
    millimetre of 0 (near at every step); on ray 2 one sample exactly on the upper bound of step 0 and a weight of exactly 0 at an
    empty sample: both have a term of 0, which the division by n_hit turns into NaN where the others become +-inf."""
    w, z, d = _random_case(4, 8, 41)
    d = torch.zeros(4)
    z = torch.linspace(0.05, 1.0, 8).repeat(4, 1) + torch.arange(4)[:, None] * 0.003
    z[1, 2], z[1, 5], z[3, 0] = 0.0007, -0.0004, 0.0009
    z[2, 6] = float(F32(0.0) + F32(_eps(0)))
    w[2, 1] = 0.0
    return w, z.float(), d


# name -> builder of (weights [N,T] fp32, z_vals [N,T] fp32, depth [N] fp32 or fp16), torch tensors on the CPU
LOS_CASES = {
    "40x768": lambda: _ladder(40, 768, 21),
    "3x260_near_then_far": lambda: _near_rows(260, far_tail=True, seed=1),
    "3x520_all_near": lambda: _near_rows(520, closest_at=515, seed=2),
    "3x130_all_near": lambda: _near_rows(130, closest_at=129, seed=3),
    "8197x8": lambda: _many_rays(far_rays=(8192, 8194, 8196)),
    "8197x8_first_ray": lambda: _many_rays(far_rays=(0,)),
    "8197x6": lambda: _ladder(8197, 6, 22, dropped=[3, 4000, 8193]),
    "5x72_half_depth": lambda: _ladder(5, 72, 23, half=True),
    "4x8_all_dropped": _all_dropped,
}
# the same cases for a float64 evaluation of the restatement: no sample ON a bound (the fp16 case has no float64 counterpart)
LOS_CASES_OFF_BOUNDS = dict(LOS_CASES)
LOS_CASES_OFF_BOUNDS.update({"40x768": lambda: _ladder(40, 768, 21, on_bounds=False),
                             "8197x6": lambda: _ladder(8197, 6, 22, dropped=[3, 4000, 8193], on_bounds=False)})
del LOS_CASES_OFF_BOUNDS["5x72_half_depth"], LOS_CASES_OFF_BOUNDS["4x8_all_dropped"]
# case -> the columns a kernel that stopped early would have read: (its wrong normaliser comes from these alone)
LOS_FIRST_CHUNKS = {"3x260_near_then_far": slice(0, 256), "3x520_all_near": slice(0, 512), "3x130_all_near": slice(0, 128)}
_los_cache = {}


def los_case(name, off_bounds=False):
    """The case as numpy-backed CPU tensors, built once and shared: do not write to them."""
    key = (name, off_bounds)
    if key not in _los_cache:
        _los_cache[key] = (LOS_CASES_OFF_BOUNDS if off_bounds else LOS_CASES)[name]()
    return _los_cache[key]


def los_reference(name, step, upstream=1.0, **kw):
    key = ("ref", name, step, upstream, tuple(sorted(kw.items())))
    if key not in _los_cache:
        w, z, d = los_case(name)
        _los_cache[key] = los_ref64(w.numpy(), z.numpy(), d.numpy(), step, ITERS, upstream, **kw)
    return _los_cache[key]


def assert_los_case(name):
    """Every builder made the situation its name promises (tests/test_loss_ref_cpu.py runs this for every case)."""
    w, z, d = los_case(name)
    N, T = z.shape
    assert w.shape == z.shape and d.shape == (N,) and w.dtype == z.dtype == torch.float32 and f"{N}x{T}" == name.split("_")[0]
    zn, dn = z.numpy(), d.numpy()
    parts = {s: _los_parts(zn, dn, s, ITERS) for s in STEPS}
    near0, empty0, bell0, n_hit = parts[0]
    on_bound = ~near0 & ~empty0
    skip = _on_bounds_mask(N, T) if name in ("40x768", "8197x6", "5x72_half_depth") else None
    if name != "4x8_all_dropped":
        for s in STEPS:
            assert los_margin(zn, dn, s, skip) >= MARGIN and n_hit > 0, (name, s, los_margin(zn, dn, s, skip))
    if skip is not None:      # the ladder cases: near samples on every ray at every step, two samples on ray 0's bounds at step 0
        assert int(on_bound.sum()) == 2 and int(on_bound[0].sum()) == 2
        for s in STEPS:
            assert int(parts[s][0].sum(1).min()) >= 1 and not parts[s][0].all() and parts[s][2].max() == 1.0
    if name in LOS_CASES_OFF_BOUNDS:
        zo, do = (t.numpy() for t in los_case(name, off_bounds=True)[1:])
        for s in STEPS:
            assert los_margin(zo, do, s) >= MARGIN
            lo64, hi64 = do.astype(F64)[:, None] - _eps(s), do.astype(F64)[:, None] + _eps(s)  # float64 bounds: the same sets
            assert np.array_equal((zo > lo64) & (zo < hi64), _los_parts(zo, do, s, ITERS)[0])
    if name == "40x768":
        assert T % 4 == 0 and T == 3 * 256
    elif name == "3x260_near_then_far":
        assert T % 4 == 0 and near0[:, :256].all() and not near0[:, 256:].any() and bell0.max() == 1.0
        assert los_bell_max(zn, dn, 0, LOS_FIRST_CHUNKS[name]) < 0.5
    elif name in ("3x520_all_near", "3x130_all_near"):
        first = LOS_FIRST_CHUNKS[name]
        assert T % 4 == (0 if name == "3x520_all_near" else 2) and near0.all()
        assert abs(bell0.max() - 0.835) < 1e-3 and np.argmax(bell0.max(0)) >= first.stop and los_bell_max(zn, dn, 0, first) < 0.5
    elif name.startswith("8197x8"):
        far = ~near0.all(1)
        assert T % 4 == 0 and N > 8192 and 0 < n_hit < N - 80 and dn[0] > 0 and (dn[8192:] > 0).all() and bell0.max() == 1.0
        assert (np.flatnonzero(far) >= 8192).all() and far.sum() == 3 if name == "8197x8" else list(np.flatnonzero(far)) == [0]
        without = float(bell0[near0].max())  # the normaliser without the far samples: exp(-0.0011^2 / (2 (0.02 / 3)^2)) = 0.986
        assert without < 0.99 and abs(los_reference(name, 0, m=without)[0] - los_reference(name, 0)[0]) > 1e-3 * los_reference(name, 0)[0]
    elif name == "8197x6":
        assert T % 4 == 2 and N > 8192 and n_hit == N - 3 and dn[8193] == 0
    elif name == "5x72_half_depth":
        assert d.dtype == torch.float16 and T % 4 == 0
        _, lo, hi = los_bounds(dn, _eps(0))
        assert np.array_equal(lo, lo.astype(F16).astype(F32)) and not np.array_equal(lo, dn.astype(F32) - F32(_eps(0)))
    elif name == "4x8_all_dropped":
        assert n_hit == 0 and near0.sum() == 3 and on_bound.sum() == 1 and on_bound[2, 6] and float(w[2, 1]) == 0.0 and empty0[2, 1]
    if name in LOS_FIRST_CHUNKS:  # the wrong normaliser is far outside the bound of the device test (1e-6)
        true, _ = los_reference(name, 0)
        wrong, _ = los_reference(name, 0, m=los_bell_max(zn, dn, 0, LOS_FIRST_CHUNKS[name]))
        one, _ = los_reference(name, 0, m=1.0)
        assert abs(wrong - true) > 1e-3 * true
        assert (one == true) if name == "3x260_near_then_far" else abs(one - true) > 1e-3 * true


def same_pattern(got, want):
    """NaN where ``want`` is NaN, inf of the same sign where it is inf, finite elsewhere."""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)))


# ==== primary losses ======================================================================================================================
KINDS = ("l1", "mse", "bce", "huber")
TRIPLES = list(itertools.product(KINDS, KINDS, KINDS))
BCE_FREE = [t for t in TRIPLES if "bce" not in t]   # 27
WITH_BCE = [t for t in TRIPLES if "bce" in t]       # 37
PRIMARY_N = (1, 255, 256, 257)
DELTA = 2.0 ** -9                                   # Huber's delta in the tests: a power of two, a multiple of LATTICE
LATTICE = 2.0 ** -12
# (smooth, (alpha_d, alpha_r, alpha_i)): both settings of rc.PRIMARY_REF_SETTINGS, and their alphas again with smooth 0 and 0.5
SETTINGS = tuple(rc.PRIMARY_REF_SETTINGS) + ((0.0, rc.PRIMARY_REF_SETTINGS[0][1]), (0.5, rc.PRIMARY_REF_SETTINGS[1][1]))
LOGITS = tuple(s * v for v in (0.0, 1e-8, 20.0, 88.0, 89.0, 104.0, 1000.0) for s in (1.0, -1.0))
# rows of the planted block
DROPPED_ROWS = slice(0, 2)
EXACT_ROW = 2
HUBER_ROWS = slice(3, 9)
LOGIT_ROWS = slice(9, 9 + 2 * len(LOGITS))
N_PLANTED = LOGIT_ROWS.stop


def upper_target(smooth, half):
    """The upper smoothing target as step_gt forms it: float32 1 - smooth, rounded to half for fp16 ground truth."""
    hi = F32(1.0) - F32(smooth)
    return F32(F16(hi)) if half else hi


def planted_block(smooth, half, delta=DELTA):
    """-> depth [P], image [P,2], gt [P,3] float32 (every gt value exact in half), P = N_PLANTED rows:

      DROPPED_ROWS  m == 0 with predictions and ground truth that are not 0: every masked product is +-0
      EXACT_ROW     e == 0 in every term: depth == gt depth, intensity == gt intensity, ray-drop == the upper smoothing target
      HUBER_ROWS    gt depth 0.5 and gt intensity 0.25; depth and intensity at gt + e for e = delta, -delta, delta + 2^-12,
                    -(delta + 2^-12), delta - 2^-12, -(delta - 2^-12).  With delta a power of two that is a multiple of 2^-12 the
                    sums and the kernel's subtraction are exact: |e| == delta on both signs, and a lattice step to either side.
                    The ray-drop prediction is the upper target + e: exact for smooth 0 and 0.5, where the target is 1 and 0.5
      LOGIT_ROWS    depth, ray-drop and intensity all at each of LOGITS = +-0, +-1e-8, +-20, +-88, +-89, +-104, +-1000 -- expf(-a) is
                    inf from a = -89 down, expf(-|a|) is 0 from |a| = 104 up -- once with m == 1, once with m == 0 (then only
                    the ray-drop term sees the value; the others see its sign on a zero)."""
    P = N_PLANTED
    depth, image, gt = np.zeros(P, F32), np.zeros((P, 2), F32), np.zeros((P, 3), F32)
    hi = upper_target(smooth, half)
    gt[:, 0], gt[:, 1], gt[:, 2] = 1.0, 0.25, 0.5
    gt[DROPPED_ROWS, 0] = 0.0
    depth[DROPPED_ROWS], image[DROPPED_ROWS] = (0.75, -0.375), ((0.3, 0.6), (-1.5, -0.125))
    depth[EXACT_ROW], image[EXACT_ROW] = 0.5, (hi, 0.25)
    step = F32(LATTICE)
    e = np.array([delta, -delta, delta + step, -(delta + step), delta - step, -(delta - step)], F32)
    assert float(delta) == float(F32(delta)) and float(delta) % LATTICE == 0
    depth[HUBER_ROWS], image[HUBER_ROWS, 0], image[HUBER_ROWS, 1] = F32(0.5) + e, hi + e, F32(0.25) + e
    v = np.array(LOGITS + LOGITS, F32)
    depth[LOGIT_ROWS], image[LOGIT_ROWS, 0], image[LOGIT_ROWS, 1] = v, v, v
    gt[LOGIT_ROWS.start + len(LOGITS):LOGIT_ROWS.stop, 0] = 0.0
    assert np.array_equal(gt.astype(F16).astype(F32), gt)
    return depth, image, gt


def primary_inputs(n, half, seed, smooth, delta=DELTA):
    """-> depth [n], image [n,2], gt [n,3] (float16 if ``half``), rays_d [n,3] as numpy arrays, and the scene scale:
    rc.loss_inputs(n, half, seed) with ``planted_block`` written over its first rows.  n below the block's size takes as many rows
    of the block as fit, starting at row ``seed`` (mod P) and wrapping, so that n = 1 meets a different planted row per seed."""
    depth, image, gt, rays_d, S = rc.loss_inputs(n, half, seed)
    depth, image, gt, rays_d = depth.numpy().copy(), image.numpy().copy(), gt.numpy().copy(), rays_d.numpy().copy()
    pd, pi, pg = planted_block(smooth, half, delta)
    rows = (np.arange(min(n, N_PLANTED)) + (seed if n < N_PLANTED else 0)) % N_PLANTED
    k = rows.size
    depth[:k], image[:k], gt[:k] = pd[rows], pi[rows], pg[rows].astype(gt.dtype)
    return depth, image, gt, rays_d, S


def _gt_terms(gt, smooth):
    """step_gt: -> m, gt_i, gt_d, gs float32 [n] (``smooth`` a float32 scalar)."""
    raw = gt.astype(F32)
    m = raw[:, 0]
    one = F32(1.0)
    if gt.dtype == F16:  # each product and each clamp bound rounded to half, then widened exactly
        gt_i, gt_d = (raw[:, 1] * m).astype(F16).astype(F32), (raw[:, 2] * m).astype(F16).astype(F32)
        lo, hi = F32(F16(smooth)), F32(F16(one - smooth))
    else:
        assert gt.dtype == F32
        gt_i, gt_d = raw[:, 1] * m, raw[:, 2] * m
        lo, hi = smooth, one - smooth
    return m, gt_i, gt_d, np.minimum(np.maximum(m, lo), hi), raw


def _criterion32(kind, a, b, delta):
    """step_criterion in numpy float32, expression by expression -> (value, d value / d a)."""
    e = a - b
    if kind == "l1":
        return np.abs(e), (e > 0).astype(F32) - (e < 0).astype(F32)
    if kind == "mse":
        return e * e, F32(2.0) * e
    if kind == "huber":
        z = np.abs(e)
        dv = np.where(e < -delta, -delta, np.where(e > delta, delta, e))
        return np.where(z < delta, F32(0.5) * z * z, delta * (z - F32(0.5) * delta)), dv
    assert kind == "bce"
    one = F32(1.0)
    with np.errstate(over="ignore", under="ignore"):
        dv = one / (one + np.exp(-a)) - b
        v = (one - b) * a - (np.minimum(a, F32(0.0)) - np.log1p(np.exp(-np.abs(a))))
    return v, dv


def primary_losses_emul(depth, image, gt, rays_d, kinds, alphas, smooth, delta, scale):
    """l4ds_primary_losses in numpy float32, every expression in the order step_primary_losses_kernel, step_gt and step_criterion
    (csrc/stepglue.hip) write it, scalars rounded to fp32 first, no contraction; ``gt`` float32 or float16; the loss through
    rc.fixed_order_sum -> dict(loss [1], g_depth [n], g_image [n,2], pts [2,n,3], gt32 [n,3]).  Where no exp or log1p is involved
    (no "bce" among ``kinds``) these are the kernel's bits; with "bce" numpy's exp / log1p stand in for the device's."""
    depth, image, rays_d = (np.ascontiguousarray(a, dtype=F32) for a in (depth, image, rays_d))
    alpha_d, alpha_r, alpha_i, smooth, delta, scale = (F32(a) for a in (*alphas, smooth, delta, scale))
    m, gt_i, gt_d, gs, raw = _gt_terms(np.asarray(gt), smooth)
    one = F32(1.0)
    p_r, p_i, p_d = image[:, 0], image[:, 1] * m, depth * m
    chain_r = None
    if kinds[1] == "bce":  # the sigmoid in front of BCE-with-logits
        with np.errstate(over="ignore", under="ignore"):
            p_r = one / (one + np.exp(-p_r))
        chain_r = (one - p_r) * p_r
    v_d, dv_d = _criterion32(kinds[0], p_d, gt_d, delta)
    v_r, dv_r = _criterion32(kinds[1], p_r, gs, delta)
    v_i, dv_i = _criterion32(kinds[2], p_i, gt_i, delta)
    acc = alpha_d * v_d + alpha_r * v_r + alpha_i * v_i
    g_r = alpha_r * dv_r * chain_r if chain_r is not None else alpha_r * dv_r
    g_image = np.stack([g_r, alpha_i * dv_i * m], -1)
    pts = np.stack([rays_d * p_d[:, None] / scale, rays_d * gt_d[:, None] / scale])
    out = dict(loss=np.array([rc.fixed_order_sum(acc)]), g_depth=alpha_d * dv_d * m, g_image=g_image, pts=pts, gt32=raw.copy())
    assert all(a.dtype == F32 for a in out.values())
    return out


def _criterion64(kind, a, b, delta):
    e = a - b
    if kind == "l1":
        return np.abs(e), np.sign(e)
    if kind == "mse":
        return e * e, 2.0 * e
    if kind == "huber":
        z = np.abs(e)
        return np.where(z < delta, 0.5 * z * z, delta * (z - 0.5 * delta)), np.clip(e, -delta, delta)
    assert kind == "bce"
    with np.errstate(over="ignore", under="ignore"):
        return (1.0 - b) * a - (np.minimum(a, 0.0) - np.log1p(np.exp(-np.abs(a)))), 1.0 / (1.0 + np.exp(-a)) - b


def primary_losses_ref64(depth, image, gt, rays_d, kinds, alphas, smooth, delta, scale, upper=None):
    """The same outputs in float64.  The ground truth's terms are taken as step_gt takes them (``_gt_terms``: float32, or rounded
    through half) and the scalars are the float32 values the kernel receives; from there on criterion, value, gradient, sum and
    points are float64.  ``upper``: the upper smoothing target to use instead of step_gt's float32 ``1 - smooth`` (a float64
    evaluation of ``lidar_loss`` takes 1 - smooth in float64, up to 2^-25 away)."""
    alpha_d, alpha_r, alpha_i, smooth32, delta, scale = (float(F32(a)) for a in (*alphas, smooth, delta, scale))
    m, gt_i, gt_d, gs, raw = (a.astype(F64) for a in _gt_terms(np.asarray(gt), F32(smooth)))
    if upper is not None:
        gs = np.minimum(np.maximum(m, float(F32(smooth))), float(upper))
    depth, image, rays_d = (np.asarray(a, dtype=F32).astype(F64) for a in (depth, image, rays_d))
    p_r, p_i, p_d = image[:, 0], image[:, 1] * m, depth * m
    chain_r = 1.0
    if kinds[1] == "bce":
        with np.errstate(over="ignore", under="ignore"):
            p_r = 1.0 / (1.0 + np.exp(-p_r))
        chain_r = (1.0 - p_r) * p_r
    v_d, dv_d = _criterion64(kinds[0], p_d, gt_d, delta)
    v_r, dv_r = _criterion64(kinds[1], p_r, gs, delta)
    v_i, dv_i = _criterion64(kinds[2], p_i, gt_i, delta)
    loss = (alpha_d * v_d + alpha_r * v_r + alpha_i * v_i).sum()
    g_image = np.stack([alpha_r * dv_r * chain_r, alpha_i * dv_i * m], -1)
    pts = np.stack([rays_d * p_d[:, None] / scale, rays_d * gt_d[:, None] / scale])
    return dict(loss=np.array([loss]), g_depth=alpha_d * dv_d * m, g_image=g_image, pts=pts, gt32=raw.astype(F32))


def deviation_units(got, want64):
    """max |got - want| in units of 2^-24 of the largest magnitude of ``want`` (0 where that is 0 and they agree)."""
    want64 = np.asarray(want64, dtype=F64)
    top = float(np.abs(want64).max()) if want64.size else 0.0
    err = float(np.abs(np.asarray(got).astype(F64) - want64).max()) if want64.size else 0.0
    return 0.0 if err == 0.0 else err / (2.0 ** -24 * top)


# Outputs a transcendental feeds, by which term carries "bce": the loss always; g_depth for the depth term; g_image for the others.
def bce_outputs(kinds):
    return {"loss"} | ({"g_depth"} if kinds[0] == "bce" else set()) | ({"g_image"} if "bce" in kinds[1:] else set())


# The largest deviation of primary_losses_emul from primary_losses_ref64 over WITH_BCE x {fp32, fp16} x PRIMARY_N x SETTINGS on
# primary_inputs, in units of 2^-24 of each output's largest magnitude, as tests/test_loss_ref_cpu.py measures, prints and checks it
# (test_emulation_against_float64): numpy's float32 exp / log1p on the CPU.  The device bound is four times these.
BCE_DEVIATION = {"loss": 3.2, "g_depth": 2.6, "g_image": 8.5}  # measured: 3.16, 2.58, 8.47


# ==== ray batch ===========================================================================================================================
PI32 = float(F32(np.pi))  # the scalar pi as an fp32 tensor expression takes it (torch's and the kernel's): 8.7e-8 above pi


def ray_batch_ref64(top, left, px, py, pose, fov, H, W, image, pi=np.pi):
    """l4ds_ray_batch as include/lidar4d_step.h states it -> inds [n] int64, rays_o [n,3] float32 (copies of the translation),
    rays_d [n,3] float64, gt [n,3] in ``image``'s dtype (None without an image).  Ray k = (patch * px + r) * py + c looks through
    row top[patch] + r and column (left[patch] + c) mod W (the non-negative remainder); inds = row * W + column whatever the row;
    a row outside [0, H) reads no pixel and its gt is 0.  Directions from the formulas in step_ray_batch_kernel's comment, in
    float64: beta = -(column - W / 2) / W * 2 pi, alpha = (fov_up - row / H * fov) / 180 * pi,
    (cos alpha cos beta, cos alpha sin beta, sin alpha) rotated by the pose.  ``pi=PI32`` evaluates the same formulas with the
    float32 rounding of pi that every fp32 evaluation multiplies by (up to 8.7e-8 on an angle of beta's size, a good part of the
    2e-7 the directions are held to): for telling that share of a deviation from the rest."""
    top, left = np.asarray(top, dtype=np.int64), np.asarray(left, dtype=np.int64)
    pose = np.asarray(pose, dtype=F32).reshape(4, 4)
    k = np.arange(top.size * px * py)
    patch, rem = k // (px * py), k % (px * py)
    row, col = top[patch] + rem // py, (left[patch] + rem % py) % W
    assert (col >= 0).all() and (col < W).all()
    inds = row * W + col
    fov_up, fov_all = float(F32(fov[0])), float(F32(fov[1]))
    beta = -(col.astype(F64) - W / 2.0) / W * 2.0 * pi
    alpha = (fov_up - row.astype(F64) / H * fov_all) / 180.0 * pi
    d = np.stack([np.cos(alpha) * np.cos(beta), np.cos(alpha) * np.sin(beta), np.sin(alpha)], -1)
    rays_d = d @ pose[:3, :3].astype(F64).T
    rays_o = np.broadcast_to(pose[:3, 3], (k.size, 3)).copy()
    gt = None
    if image is not None:
        image = np.asarray(image)
        gt = np.zeros((k.size, 3), dtype=image.dtype)
        inside = (row >= 0) & (row < H)
        gt[inside] = image.reshape(-1, 3)[inds[inside]]
    return inds, rays_o, rays_d, gt
