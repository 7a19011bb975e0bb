"""Reader of the reference's preprocessed KITTI-360 layout (the on-disk formats next to the path).
Mirror of data/kitti360_dataset.py:14-209 -- same constructor fields, attributes and per-step dict -- so that
``main_lidar4d.py``'s ``KITTI360Dataset(...).dataloader()`` can be pointed here unchanged.

Layout (written by the reference's preprocess scripts):
  ``<root>/transforms_<seq>_<split>.json``  {"h_lidar", "w_lidar", "frames": [{"lidar2world": 4x4, "lidar_file_path",
                                             "frame_id"}, ...]}
  ``<root>/<lidar_file_path>.npy``          range view [H, W, 3] float: (unused, intensity, depth in metres; 0 = no return)

Frames are parsed once and moved to ``device`` (the GPU's HBM when ``preload``); ``collate`` cuts one frame's batch with
lidar4d_amd.data.get_lidar_rays, as the reference's loader does.

The dataset also speaks ``lidar4d_amd.trainer.Trainer``'s dataset protocol (``num_frames``, ``frames``, ``sequence_index``,
``next_frame``, ``batch_for``, ``batch``, ``frame``, ``scale`` / ``fov`` / ``num_rays`` / ``gen``): a preloaded dataset on a HIP
device draws a step's batch with two ``randint``s and one launch (``ops.ray_batch_patches``, include/lidar4d_step.h) that keeps
the ground truth in the dtype it was preloaded in -- fp16 by default, as in the reference.
"""
import json
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, RandomSampler

from .data import _patch_shape, draw_ray_batch, get_lidar_rays

# first and last frame id of the sequences the reference knows (kitti360_dataset.py:29-71)
SEQUENCE_FRAMES = {
    "1538": (1538, 1601), "1728": (1728, 1791), "1908": (1908, 1971), "3353": (3353, 3416),
    "2350": (2350, 2400), "4950": (4950, 5000), "8120": (8120, 8170), "10200": (10200, 10250),
    "10750": (10750, 10800), "11400": (11400, 11450),
}


class KITTI360Dataset:
    def __init__(self, device="cpu", split="train", root_path="data/kitti360", sequence_id="4950", preload=True, scale=1,
                 offset=(), fp16=True, patch_size_lidar=1, num_rays_lidar=4096, fov_lidar=(), num_frames=None, seed=0):
        """The reference's arguments, then: num_frames, the length of the SEQUENCE (default: frame_end - frame_start + 1, 51 for
        4950 as in configs/kitti360_4950.txt) -- ``len(self)`` is the number of frames this split holds; seed, of the device
        generator ``gen`` that ``batch_for`` draws pixels from."""
        if str(sequence_id) not in SEQUENCE_FRAMES:
            raise ValueError(f"Invalid sequence id: {sequence_id}")
        self.device, self.root_path, self.sequence_id = device, root_path, str(sequence_id)
        self.preload, self.scale, self.offset, self.fp16 = preload, scale, list(offset), fp16
        self.patch_size_lidar, self.fov_lidar = patch_size_lidar, list(fov_lidar)
        self.frame_start, self.frame_end = SEQUENCE_FRAMES[self.sequence_id]

        # 'refine' reads the training frames but serves whole frames (U-Net refinement, runner.py:818-863)
        self.training = split in ("train", "all", "trainval")
        self.num_rays_lidar = num_rays_lidar if self.training else -1
        self.split = "train" if split == "refine" else split

        with open(os.path.join(root_path, f"transforms_{self.sequence_id}_{self.split}.json")) as fh:
            meta = json.load(fh)
        self.H = int(meta["h"]) if "h" in meta and "w" in meta else None
        self.W = int(meta["w"]) if "h" in meta and "w" in meta else None
        self.H_lidar, self.W_lidar = int(meta["h_lidar"]), int(meta["w_lidar"])

        frames = sorted(meta["frames"], key=lambda fr: fr["lidar_file_path"])
        span = self.frame_end - self.frame_start
        poses = np.stack([np.asarray(fr["lidar2world"], dtype=np.float32) for fr in frames])
        times = np.asarray([(fr["frame_id"] - self.frame_start) / span for fr in frames], dtype=np.float32)
        images = []
        for fr in frames:
            view = np.load(os.path.join(root_path, fr["lidar_file_path"]))       # [H, W, 3]
            depth = view[:, :, 2]
            returned = np.where(depth == 0.0, 0.0, 1.0)
            images.append(np.stack([returned, view[:, :, 1], depth * self.scale], axis=-1))
        # scene normalisation of the sensor positions (configs/kitti360_*.txt: offset, scale); the offset list makes the
        # arithmetic float64 before it is stored back as float32, like the reference's numpy expression
        off = np.asarray(self.offset, dtype=np.float64) if len(self.offset) else np.zeros(3)
        poses[:, :3, 3] = (poses[:, :3, 3] - off) * self.scale
        self.poses_lidar = torch.from_numpy(poses)                               # [N, 4, 4]
        self.images_lidar = torch.from_numpy(np.stack(images)).float()           # [N, H, W, 3]
        self.times = torch.from_numpy(times).view(-1, 1)                         # [N, 1]
        if preload:
            self.poses_lidar = self.poses_lidar.to(device)
            self.images_lidar = self.images_lidar.to(torch.half if fp16 else torch.float).to(device)
            self.times = self.times.to(device)
        self.intrinsics_lidar = self.fov_lidar

        # ---- the trainer's dataset protocol ----
        self.num_frames = int(num_frames) if num_frames is not None else self.frame_end - self.frame_start + 1
        self.fov, self.num_rays = self.fov_lidar, self.num_rays_lidar
        self.times_host = [float(t) for t in times]  # the fp32 times, exactly
        # frame_index(time, num_frames) of every held frame (runner.py:949), once, on the host: an fp32 product, truncated
        self._sequence_index = [int(np.float32(t) * np.float32(self.num_frames - 1)) for t in times]
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)
        self._order = iter(())
        # [N, 1, 1] next to the images: a step's ``time`` is a view of it (no host-to-device copy inside a captured step)
        self._times_dev = torch.from_numpy(times).view(-1, 1, 1).to(device) if preload else None

    def collate(self, index):
        """index: list with one frame number (the loader's batch size is 1) -> the reference's per-step dict."""
        B = len(index)
        poses = self.poses_lidar[index].to(self.device)
        rays = get_lidar_rays(poses, self.intrinsics_lidar, self.H_lidar, self.W_lidar, self.num_rays_lidar,
                              self.patch_size_lidar)
        images = self.images_lidar[index].to(self.device)
        if self.training:  # ground truth of the drawn pixels only
            C = images.shape[-1]
            images = torch.gather(images.view(B, -1, C), 1, rays["inds"].unsqueeze(-1).expand(-1, -1, C))
        return {"H_lidar": self.H_lidar, "W_lidar": self.W_lidar, "rays_o_lidar": rays["rays_o"],
                "rays_d_lidar": rays["rays_d"], "images_lidar": images, "time": self.times[index].to(self.device),
                "poses_lidar": poses}

    def dataloader(self):
        loader = DataLoader(list(range(len(self))), batch_size=1, collate_fn=self.collate, shuffle=self.training,
                            num_workers=0)
        loader._data = self
        loader.has_gt = self.images_lidar is not None
        return loader

    def __len__(self):
        return len(self.poses_lidar)

    # ---- the trainer's dataset protocol (lidar4d_amd.trainer.Trainer) ------------------------------------------------------------
    def frames(self):
        """The held frames, as ``batch_for`` / ``frame`` / ``sequence_index`` number them."""
        return range(len(self))

    def sequence_index(self, k):
        """Where held frame ``k`` sits in the sequence: ``frame_index(times[k], num_frames)``, the key of its point clouds
        (runner.py:949) and what selects its time slices."""
        return self._sequence_index[k]

    def next_frame(self):
        """The frame of the next training step: a permutation of the held frames per epoch out of
        ``torch.utils.data.RandomSampler``, i.e. the order of the reference's loader (shuffle=True, batch size 1) for the same
        torch seed.  Host-side: no device sync."""
        for _ in range(2):
            for k in self._order:
                return int(k)
            self._order = iter(RandomSampler(range(len(self))))
        raise ValueError("KITTI360Dataset.next_frame: the split holds no frame")

    @property
    def device_batches(self):
        """``batch_for`` draws on the device and copies nothing from the host (what a captured step needs): preloaded there."""
        px = _patch_shape(self.patch_size_lidar)[0]
        return bool(self.preload) and torch.device(self.device).type == "cuda" and self.num_rays_lidar > 0 and px > 0

    def batch_for(self, k):
        """One training step's dict for held frame ``k``: the reference's keys (``collate``) plus ``index`` and ``time_host``.
        Preloaded on a HIP device: the two ``randint``s of get_lidar_rays from ``gen``, then one l4ds_ray_batch launch; the
        ground truth keeps the dtype it was preloaded in.  Otherwise the torch route (get_lidar_rays + gather)."""
        H, W = self.H_lidar, self.W_lidar
        extra = {"index": [k], "time_host": self.times_host[k]}
        if self.device_batches:
            rays_o, rays_d, images = draw_ray_batch("KITTI360Dataset.batch_for", self.gen, self.num_rays_lidar, self.patch_size_lidar,
                                                    self.poses_lidar[k], self.intrinsics_lidar, H, W, self.images_lidar[k])
            return {"H_lidar": H, "W_lidar": W, "rays_o_lidar": rays_o, "rays_d_lidar": rays_d, "images_lidar": images,
                    "time": self._times_dev[k], "poses_lidar": self.poses_lidar[k:k + 1], **extra}
        poses = self.poses_lidar[[k]].to(self.device)
        rays = get_lidar_rays(poses, self.intrinsics_lidar, H, W, self.num_rays_lidar, self.patch_size_lidar, generator=self.gen)
        images = self.images_lidar[[k]].to(self.device)
        if self.num_rays_lidar > 0:
            images = torch.gather(images.view(1, -1, 3), 1, rays["inds"].unsqueeze(-1).expand(-1, -1, 3))
        return {"H_lidar": H, "W_lidar": W, "rays_o_lidar": rays["rays_o"], "rays_d_lidar": rays["rays_d"], "images_lidar": images,
                "time": self.times[[k]].to(self.device), "poses_lidar": poses, **extra}

    def batch(self, frame=None):
        """``batch_for`` the given held frame, or the next one of the epoch's permutation."""
        return self.batch_for(self.next_frame() if frame is None else frame)

    def frame(self, k):
        """Every ray of held frame ``k`` with its ground truth [1, H, W, 3], as ``collate`` serves a non-training split."""
        poses = self.poses_lidar[[k]].to(self.device)
        rays = get_lidar_rays(poses, self.intrinsics_lidar, self.H_lidar, self.W_lidar, -1)
        return {"H_lidar": self.H_lidar, "W_lidar": self.W_lidar, "rays_o_lidar": rays["rays_o"], "rays_d_lidar": rays["rays_d"],
                "images_lidar": self.images_lidar[[k]].to(self.device), "time": self.times[[k]].to(self.device), "poses_lidar": poses,
                "index": [k], "time_host": self.times_host[k]}
