"""Point-cloud evaluation on the device.  Mirror of the reference's ``fscore`` and ``PointsMeter``
(utils/metrics.py:13-27, 224-274): range image -> points (lidar4d_amd/convert.py instead of numpy) -> chamfer distance
(lidar4d_amd/chamfer.py instead of the CUDA extension) -> chamfer distance + F-score at 0.05 (squared-distance
threshold, as the reference uses it).  Nothing leaves the GPU until ``measure()``.

``DepthMeter`` and ``IntensityMeter`` (utils/metrics.py:30-169: RMSE, MedAE, LPIPS, SSIM, PSNR of a rendered image) follow the
same rule: where the reference copies every frame to the host for numpy and skimage, the four error statistics are one call
into liblidar4d_eval.so (include/lidar4d_eval.h, csrc/evalmeter.hip) on the caller's stream.
"""
import numpy as np
import torch

from . import _eval_lib, ops
from .chamfer import chamfer_3DDist
from .convert import pano_to_lidar


def fscore(dist1, dist2, threshold=0.001):
    """utils/metrics.py:13-27.  dist1 [B, n] / dist2 [B, m]: SQUARED nearest-neighbour distances of the two directions
    (so ``threshold`` is a squared distance too).  Returns (F-score, precision, recall), each [B]; F is 0 where both
    precision and recall are 0."""
    precision = (dist1 < threshold).float().mean(dim=1)
    recall = (dist2 < threshold).float().mean(dim=1)
    denom = precision + recall
    f = torch.where(denom > 0, 2 * precision * recall / denom.clamp_min(1e-30), torch.zeros_like(denom))
    return f, precision, recall


class PointsMeter:
    def __init__(self, scale, intrinsics):
        self.V = []
        self.N = 0
        self.scale = scale
        self.intrinsics = intrinsics

    def clear(self):
        self.V = []
        self.N = 0

    def update(self, preds, truths):
        """preds, truths: [B, H, W] range images in scene units (depth * scale); only element 0 is used, like the
        reference (utils/metrics.py:253-254)."""
        preds = preds / self.scale
        truths = truths / self.scale
        pred_lidar = pano_to_lidar(preds[0], self.intrinsics)
        gt_lidar = pano_to_lidar(truths[0], self.intrinsics)
        dist1, dist2, _, _ = chamfer_3DDist()(pred_lidar[None], gt_lidar[None])
        if pred_lidar.shape[0] == 0 or gt_lidar.shape[0] == 0:
            # a degenerate frame (e.g. every predicted ray-drop <= 0.5 early in training): record the worst value of both
            # metrics instead of aborting the evaluation (the mean over an empty cloud would be nan)
            self.V.append(torch.tensor([float("inf"), 0.0], device=preds.device))
            self.N += 1
            return
        chamfer_dis = dist1.mean() + dist2.mean()
        f_score, _, _ = fscore(dist1, dist2, 0.05)
        self.V.append(torch.stack([chamfer_dis, f_score[0]]))  # stays on the device
        self.N += 1

    def measure(self):
        assert self.N == len(self.V)
        return torch.stack(self.V).mean(0).cpu().numpy().astype(np.float64)

    def report(self):
        return f"CD f-score = {self.measure()}"


class RaydropMeter:
    """utils/metrics.py:172-226: RMSE, accuracy and F1 of the ray-drop probability image against the 0/1 ground truth,
    thresholded at ``ratio``.  Torch on whatever device the inputs live on; one host transfer in ``measure()``."""

    def __init__(self, ratio=0.5):
        self.V = []
        self.N = 0
        self.ratio = ratio

    def clear(self):
        self.V = []
        self.N = 0

    def update(self, preds, truths):
        preds = torch.as_tensor(preds).detach().double()
        truths = torch.as_tensor(truths).detach().to(preds)
        rmse = ((truths - preds) ** 2).mean().sqrt()
        hit = (preds > self.ratio).to(preds)
        acc = (hit == truths).double().mean()
        tp = ((truths == 1) & (hit == 1)).sum().double()
        fp = ((truths == 0) & (hit == 1)).sum().double()
        fn = ((truths == 1) & (hit == 0)).sum().double()
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        f1 = 2 * (precision * recall) / (precision + recall)  # nan when nothing is predicted / present, like the reference
        self.V.append(torch.stack([rmse, acc, f1]))
        self.N += 1

    def measure(self):
        assert self.N == len(self.V)
        return torch.stack(self.V).mean(0).cpu().numpy()

    def report(self):
        return f"Rdrop_error (RMSE, Acc, F1) = {self.measure()}"


def _device_only(t, name):
    if not t.is_cuda:
        ops._chk(t, None, name)  # raises HipExtensionError: there is no CPU path


def image_errors(pred, gt, lo, hi):
    """pred, gt: [H, W] fp32 HIP tensors -> [4] fp64 on the device: rmse, medae, ssim, psnr of the images clamped to
    [lo, hi] (l4de_image_errors; H, W >= 7).  No host synchronisation; the inputs are left as they are."""
    _device_only(pred, "pred"), _device_only(gt, "gt")
    if pred.dim() != 2 or pred.shape != gt.shape:
        raise ValueError(f"image_errors: expected two [H, W] images of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    pred = pred.detach().to(torch.float32).contiguous()
    gt = gt.detach().to(torch.float32).contiguous()
    H, W = int(pred.shape[0]), int(pred.shape[1])
    out = torch.empty(4, dtype=torch.float64, device=pred.device)
    ws = torch.empty(max(8, int(_eval_lib.lib().l4de_image_errors_workspace(H, W))), dtype=torch.uint8, device=pred.device)
    _eval_lib.call("l4de_image_errors", ops._p(pred), ops._p(gt), H, W, float(lo), float(hi), ops._p(out), ops._p(ws),
                   ops._stream())
    return out


class _ImageMeter:
    """What DepthMeter and IntensityMeter share (the reference spells the class out twice).  V holds one device vector
    [rmse, medae, lpips, ssim, psnr] (fp64) per update."""
    lo, hi, label = 1e-6, 1.0, ""

    def __init__(self, scale, lpips_fn=None):
        self.V = []
        self.N = 0
        self.scale = scale
        # the reference builds lpips.LPIPS(net='alex') here and ignores the argument; the AlexNet weights are no part of this
        # package, so the slot is NaN unless the caller brings a function with LPIPS's call signature
        self.lpips_fn = lpips_fn

    def clear(self):
        self.V = []
        self.N = 0

    def update(self, preds, truths):
        """preds, truths: [1, H, W] HIP tensors (the reference's squeeze(0) means one image).  Not modified."""
        for name, t in (("preds", preds), ("truths", truths)):
            if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] != 1:
                raise ValueError(f"{name}: expected a [1, H, W] tensor, got {tuple(getattr(t, 'shape', ()))}")
            _device_only(t, name)
        pred = (preds.detach() / self.scale)[0]
        gt = (truths.detach() / self.scale)[0]
        err = image_errors(pred, gt, self.lo, self.hi)
        lp = torch.full((1,), float("nan"), dtype=torch.float64, device=err.device)
        if self.lpips_fn is not None:
            lo, hi = torch.tensor(self.lo, dtype=pred.dtype, device=pred.device), torch.tensor(self.hi, dtype=pred.dtype, device=pred.device)
            clamp = lambda x: torch.where(x < lo, lo, torch.where(x > hi, hi, x))  # (keeps NaN, like the kernel)
            lp = torch.as_tensor(self.lpips_fn(clamp(pred.float()), clamp(gt.float()), normalize=True)).to(err).reshape(1)
        self.V.append(torch.cat([err[:2], lp, err[2:]]))
        self.N += 1

    def measure(self):
        assert self.N == len(self.V)
        return torch.stack(self.V).mean(0).cpu().numpy().astype(np.float64)

    def report(self):
        return f"{self.label} = {self.measure()}"


class DepthMeter(_ImageMeter):
    """utils/metrics.py:30-98; depth in metres after the division by ``scale``, clamped to [1e-6, 80]."""
    lo, hi, label = 1e-6, 80.0, "Depth_error"


class IntensityMeter(_ImageMeter):
    """utils/metrics.py:101-169; intensity clamped to [1e-6, 1]."""
    lo, hi, label = 1e-6, 1.0, "Inten_error"
