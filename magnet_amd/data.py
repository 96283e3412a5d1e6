"""Dataset-free host side of the path (row N4 of SURVEY.md §8f): camera-intrinsics producer and a loader for
ScanNet-format scene folders, yielding exactly what the reference's loaders hand to `validate()` /
`MAGNET.forward` (reference: data/dataloader_scannet.py:16-217, utils/utils.py:64-98).

    <root>/<scene>/color/<i>.jpg   depth/<i>.png (uint16 millimetres)   pose/<i>.txt (4x4 cam->world)
                   intrinsic/intrinsic_color.txt (4x4)

No torchvision, no dataset split files, no JSON side tables: the raw image size is read from the first colour image
unless given.  Everything here is host code feeding the device path; nothing is timed by bench.py.
"""
from __future__ import annotations

import dataclasses
import os
import random
import typing

import numpy as np
import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def read_matrix_txt(path: str) -> np.ndarray:
    """4x4 float64 matrix from a whitespace-separated text file (first four rows)."""
    m = np.eye(4)
    with open(path, "r") as f:
        rows = [ln.split() for ln in f.read().strip().splitlines()[:4]]
    for i, r in enumerate(rows):
        m[i, :] = [float(x) for x in r[:4]]
    return m


def read_pose_txt(path: str) -> np.ndarray:
    """ScanNet stores cam->world; the model wants world->cam (dataloader_scannet.py:16-28).  A lost pose (-inf entries)
    inverts to NaN, which `preprocess.data_preprocess` turns into is_valid = 0, like the reference (utils.py:84-94)."""
    with np.errstate(all="ignore"):
        try:
            return np.linalg.inv(read_matrix_txt(path))
        except np.linalg.LinAlgError:
            return np.full((4, 4), np.nan)


def cam_intrinsics(K: np.ndarray, raw_w: int, raw_h: int, dpv_h: int, dpv_w: int, crop=(0, 0), with_table: bool = True) -> dict:
    """K (>=3x3, pixels of the image the network sees BEFORE any crop) -> {'intM' (3,3), 'unit_ray_array_2D' (3, dpv_h*dpv_w),
    'ray_params' (8,) float64}: intrinsics scaled to the matching grid and the ray ((x+0.5)*sx - cx + left)/fx,
    ((y+0.5)*sy - cy + top)/fy, 1 of every grid pixel, row-major (float64 math, one cast).
      ScanNet / 7-Scenes (dataloader_scannet.py:113-153, dataloader_7scenes.py:72-116): raw_w x raw_h = the raw image, no crop.
      KITTI (dataloader_kitti.py:83-127): raw_w x raw_h = the CROPPED network input (1216 x 352), crop = (left, top) margins of the
      KB crop inside the raw frame — see cam_intrinsics_kitti.
    'ray_params' = (fx, fy, cx, cy, sx, sy, left, top): what the kernel needs to generate the rays itself (the 12*h*w-byte
    table then never exists: pass with_table=False)."""
    K = np.asarray(K, dtype=np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    left, top = float(crop[0]), float(crop[1])
    intM = np.zeros((3, 3))
    intM[2, 2] = 1.0
    intM[0, 0], intM[1, 1] = fx * (dpv_w / raw_w), fy * (dpv_h / raw_h)
    intM[0, 2], intM[1, 2] = (cx - left) * (dpv_w / raw_w), (cy - top) * (dpv_h / raw_h)
    sx, sy = raw_w / dpv_w, raw_h / dpv_h
    out = {"intM": torch.from_numpy(intM.astype(np.float32)),
           "ray_params": torch.tensor([fx, fy, cx, cy, sx, sy, left, top], dtype=torch.float64)}
    if with_table:
        xs = np.arange(dpv_w, dtype=np.float64)[None, :] + 0.5
        ys = np.arange(dpv_h, dtype=np.float64)[:, None] + 0.5
        rays = np.ones((3, dpv_h, dpv_w))
        rays[0] = (xs * sx - cx + left) / fx
        rays[1] = (ys * sy - cy + top) / fy
        out["unit_ray_array_2D"] = torch.from_numpy(rays.reshape(3, -1).astype(np.float32))
    return out


def cam_intrinsics_kitti(K_cam2: np.ndarray, raw_w: int, raw_h: int, dpv_h: int, dpv_w: int, img_h: int = 352, img_w: int = 1216,
                         with_table: bool = True) -> dict:
    """KITTI (dataloader_kitti.py:94-127): the network input is the 1216 x 352 KB crop of the raw_w x raw_h frame
    (top margin raw_h - 352, left margin (raw_w - 1216) / 2, both truncated to int); K_cam2 is the raw calibration."""
    top = int(raw_h - img_h)
    left = int((raw_w - img_w) / 2)
    return cam_intrinsics(K_cam2, img_w, img_h, dpv_h, dpv_w, crop=(left, top), with_table=with_table)


def cam_intrinsics_7scenes(dpv_h: int, dpv_w: int, img_h: int = 480, img_w: int = 640, with_table: bool = True) -> dict:
    """7-Scenes (dataloader_7scenes.py:83-116): fixed fx = fy = 585, principal point (320, 240) of the 640 x 480 frames."""
    K = np.array([[585.0, 0.0, 320.0], [0.0, 585.0, 240.0], [0.0, 0.0, 1.0]])
    return cam_intrinsics(K, img_w, img_h, dpv_h, dpv_w, with_table=with_table)


def window_indices(center: int, n_views: int, window_radius: int, exists) -> list:
    """Frame indices of the local window, reference frame in the middle (dataloader_scannet.py:81-89,160-165): offsets
    k * (radius // (n_views // 2)), k = -n/2..n/2; a missing neighbour is mirrored to the other side, half a step closer."""
    step = window_radius // (n_views // 2)
    out = []
    for k in range(-(n_views // 2), n_views // 2 + 1):
        off = k * step
        if exists(center + off):
            out.append(center + off)
        else:
            out.append(center - off - int(np.sign(off)) * int(step * 0.5))
    return out


# ---- training-mode augmentation (dataloader_scannet.py:171-200,219-232, dataloader_scannet_D.py:80-156, and their KITTI twins) ----
@dataclasses.dataclass(frozen=True)
class AugmentSpec:
    """Which of the reference loaders' augmentations a folder draws.  color: gamma in [0.9, 1.1], brightness in `brightness`
    ((0.75, 1.25) for ScanNet and 7-Scenes, (0.9, 1.1) for KITTI) and three channel factors in [0.9, 1.1], with probability 1/2;
    flip: a horizontal flip with probability 1/2; crop_hw: a random (height, width) window of the resized image.  The loaders'
    rotation (data_augmentation_rotate: Pillow's affine transform in double precision) is out of scope: there is no field for it."""
    color: bool = False
    brightness: tuple = (0.75, 1.25)
    flip: bool = False
    crop_hw: tuple | None = None


class Augment(typing.NamedTuple):
    """One sample's draw.  color: None or (gamma, brightness, (c_r, c_g, c_b)); flip: bool; window: None (the whole resized image) or
    the (x, y) origin of the crop window in the (flipped) resized image."""
    color: tuple | None = None
    flip: bool = False
    window: tuple | None = None


def draw_augment(spec, py_rng, np_rng, resized_hw):
    """The reference's draws in its order and from the same kinds of generator (py_rng: a random.Random, np_rng: a
    numpy.random.RandomState): flip coin (dataloader_scannet_D.py:92-95), crop x then y with randint (:134-135), colour coin (:108),
    gamma, brightness (:142-146), then the three colours from numpy (:150).  A draw that `spec` switches off consumes nothing."""
    flip = bool(py_rng.random() > 0.5) if spec.flip else False
    window = None
    if spec.crop_hw is not None:
        ch, cw = (int(v) for v in spec.crop_hw)
        if ch < 1 or cw < 1 or ch > resized_hw[0] or cw > resized_hw[1]:
            raise ValueError(f"draw_augment: a crop of {(ch, cw)} does not fit the resized image {tuple(resized_hw)}")
        x = py_rng.randint(0, resized_hw[1] - cw)
        window = (x, py_rng.randint(0, resized_hw[0] - ch))
    color = None
    if spec.color and py_rng.random() > 0.5:
        gamma = py_rng.uniform(0.9, 1.1)
        brightness = py_rng.uniform(*spec.brightness)
        color = (gamma, brightness, tuple(float(c) for c in np_rng.uniform(0.9, 1.1, size=3)))
    return Augment(color, flip, window)


def augment_rngs(seed, epoch, index):
    """The two generators of one item, seeded from (seed, epoch, item index) alone: a sample's draw does not depend on the worker
    count, on the order of iteration or on which path prepares it."""
    key = [int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, int(index) & 0xFFFFFFFF]
    return random.Random((key[0] << 64) | (key[1] << 32) | key[2]), np.random.RandomState(key)


def augment_image(image, gamma, brightness, colors):
    """The loaders' colour augmentation of an (H, W, 3) float32 image in [0, 1], with their dtypes (dataloader_scannet.py:219-232):
    float32 power and product, an in-place product with a float64 colour image (computed in float64, rounded to float32), a clip."""
    image_aug = image ** gamma
    image_aug = image_aug * brightness
    white = np.ones((image.shape[0], image.shape[1]))
    image_aug *= np.stack([white * colors[i] for i in range(3)], axis=2)
    return np.clip(image_aug, 0, 1)


def _check_spec(augment, multi_view):
    if augment is None:
        return None
    if not isinstance(augment, AugmentSpec):
        raise TypeError(f"augment must be an AugmentSpec or None, got {type(augment).__name__}")
    if multi_view and (augment.flip or augment.crop_hw is not None):
        raise ValueError("a multi-view folder takes the colour augmentation only, as the reference's multi-view loaders do: a flip or a "
                         "crop would invalidate the intrinsics and the poses of the window")
    return augment


class ScanNetFolder:
    """samples: list of (scene_name, frame_index).  __getitem__ -> (data_array, cam_intrins): a list of n_views + 1 dicts
    {'img' (3,H,W) normalised fp32, 'gt_dmap' (1,H,W) metres for the reference frame else 0.0, 'extM' (4,4) float64,
    'scene_name', 'img_idx'} and the intrinsics dict — the structure of dataloader_scannet.py:155-217.
    raw_images=True (opt-in): 'img' is the decoded frame itself, a uint8 (Hraw, Wraw, 3) tensor, neither resized nor normalised —
    magnet_amd.ingest.ImagePrep does both on the device, to the same bits.  Everything else of an item is unchanged.
    augment (opt-in; an AugmentSpec with colour only): the training mode of the reference's multi-view loader (:171-194), one colour
    draw per sample, shared by its views, from generators seeded by (seed, epoch, item index); set_epoch(e) before each epoch.  The
    host path applies it.  With raw_images=True the frames stay untouched, every dict carries the draw under 'aug', and the reference
    frame's dict carries the decoded uint16 depth map under 'gt_dmap_raw' in place of 'gt_dmap': magnet_amd.ingest.TrainPrep
    prepares both on the device, to the host path's bits.  The loaders' rotation augmentation is out of scope (AugmentSpec)."""

    def __init__(self, root, samples, n_views=4, window_radius=20, input_hw=(480, 640), dpv_hw=(120, 160), raw_wh=None, raw_images=False,
                 augment=None, seed=0):
        from PIL import Image  # noqa: F401  (fail early if Pillow is missing)
        self.root, self.samples = root, list(samples)
        self.n_views, self.window_radius = n_views, window_radius
        self.img_h, self.img_w = input_hw
        self.dpv_h, self.dpv_w = dpv_hw
        self.raw_wh = dict(raw_wh or {})
        self.center = n_views // 2
        self.raw_images = bool(raw_images)
        self.augment, self.seed, self.epoch = _check_spec(augment, multi_view=True), int(seed), 0

    def __len__(self):
        return len(self.samples)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _scene(self, name):
        return os.path.join(self.root, name)

    # file naming of the format; SevenScenesFolder overrides these
    def _color(self, sdir, k):
        return os.path.join(sdir, "color", f"{k}.jpg")

    def _depth(self, sdir, k):
        return os.path.join(sdir, "depth", f"{k}.png")

    def _pose(self, sdir, k):
        return os.path.join(sdir, "pose", f"{k}.txt")

    def _intrinsics(self, scene, sdir, idx):
        raw_w, raw_h = self._raw_wh(scene, idx)
        return cam_intrinsics(read_matrix_txt(os.path.join(sdir, "intrinsic", "intrinsic_color.txt")), raw_w, raw_h, self.dpv_h, self.dpv_w)

    def _split(self, sample):
        scene, idx = sample
        return scene, self._scene(scene), int(idx)

    depth_divisor, depth_invalid = 1000.0, None                                # what ingest.TrainPrep needs to restate _depth_metres

    def _depth_metres(self, raw):
        return raw.astype(np.float32) / 1000.0                                  # uint16 millimetres

    def _raw_wh(self, scene, any_idx):
        if scene not in self.raw_wh:
            from PIL import Image
            with Image.open(self._color(self._scene(scene), any_idx)) as im:
                self.raw_wh[scene] = im.size                                   # (W, H)
        return self.raw_wh[scene]

    def __getitem__(self, i):
        from PIL import Image
        scene, sdir, idx = self._split(self.samples[i])
        frames = window_indices(idx, self.n_views, self.window_radius, lambda k: os.path.exists(self._color(sdir, k)))
        intr = self._intrinsics(scene, sdir, idx)
        mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
        aug = None if self.augment is None else draw_augment(self.augment, *augment_rngs(self.seed, self.epoch, i), (self.img_h, self.img_w))
        data_array = []
        for j, k in enumerate(frames):
            with Image.open(self._color(sdir, k)) as im:
                rgb = im.convert("RGB")
                if not self.raw_images:
                    rgb = rgb.resize((self.img_w, self.img_h), resample=Image.BILINEAR)
            if self.raw_images:
                img = torch.from_numpy(np.array(rgb, dtype=np.uint8))           # (Hraw, Wraw, 3), a copy the tensor owns
            else:
                img = np.asarray(rgb).astype(np.float32) / 255.0
                if aug is not None and aug.color is not None:
                    img = augment_image(img, *aug.color)
                img = torch.from_numpy(img).permute(2, 0, 1)
                img = (img - mean) / std
            entry = {"img": img, "gt_dmap": 0.0, "extM": read_pose_txt(self._pose(sdir, k)), "scene_name": scene, "img_idx": str(k)}
            if j == self.center:
                with Image.open(self._depth(sdir, k)) as dm:
                    if self.raw_images and aug is not None:
                        del entry["gt_dmap"]
                        entry["gt_dmap_raw"] = torch.from_numpy(np.array(dm, dtype=np.uint16))       # (Hd, Wd), decoded only
                    else:
                        d = self._depth_metres(np.asarray(dm.resize((self.img_w, self.img_h), resample=Image.NEAREST)))
                        entry["gt_dmap"] = torch.from_numpy(d)[None]
            if self.raw_images and aug is not None:
                entry["aug"] = aug
            data_array.append(entry)
        return data_array, intr


class SevenScenesFolder(ScanNetFolder):
    """7-Scenes layout (data/dataloader_7scenes.py): <root>/<scene>/seq-XX/frame-XXXXXX.{color.png,depth.png,pose.txt}; samples are
    (scene, sequence id, frame index); the published intrinsics fx = fy = 585, c = (320, 240) apply to the 640x480 frames and are
    scaled by the INPUT size, as the reference does (:78-100)."""

    def _split(self, sample):
        scene, seq, idx = sample
        return "%s_seq-%02d" % (scene, int(seq)), os.path.join(self.root, scene, "seq-%02d" % int(seq)), int(idx)

    depth_invalid = 65535

    def _depth_metres(self, raw):
        raw = raw.copy()
        raw[raw == 65535] = 0                                                    # the sensor's "no measurement" code (:150)
        return raw.astype(np.float32) / 1000.0

    def _color(self, sdir, k):
        return os.path.join(sdir, "frame-%06d.color.png" % k)

    def _depth(self, sdir, k):
        return os.path.join(sdir, "frame-%06d.depth.png" % k)

    def _pose(self, sdir, k):
        return os.path.join(sdir, "frame-%06d.pose.txt" % k)

    def _intrinsics(self, scene, sdir, idx):
        K = np.eye(3); K[0, 0] = K[1, 1] = 585.0; K[0, 2], K[1, 2] = 320.0, 240.0
        return cam_intrinsics(K, self.img_w, self.img_h, self.dpv_h, self.dpv_w)


class ScanNetFrames(ScanNetFolder):
    """Single-view training items, the structure of dataloader_scannet_D.py:73-127: samples as ScanNetFolder's, __getitem__ ->
    {'img' (3,H,W) normalised fp32, 'depth' (1,H,W) metres, 'scene_name', 'img_idx'}.  augment: an AugmentSpec with any of flip, crop
    and colour, applied in the reference's order (:91-109): flip of image and depth, /255 and /1000, the crop window of both, colour,
    normalisation; with crop_hw the item is (3, crop_h, crop_w) / (1, crop_h, crop_w).  Draws as ScanNetFolder's: seeded by
    (seed, epoch, item index).  raw_images=True: 'img' is the decoded uint8 frame (Hraw, Wraw, 3), 'depth' the decoded uint16 map
    (Hd, Wd), and 'aug' the draw (an all-default Augment without a spec), for magnet_amd.ingest.TrainPrep.  The loaders' rotation
    augmentation is out of scope (AugmentSpec).  SevenScenesFrames is the 7-Scenes variant."""

    def __init__(self, root, samples, input_hw=(480, 640), raw_images=False, augment=None, seed=0):
        ScanNetFolder.__init__(self, root, samples, input_hw=input_hw, raw_images=raw_images, seed=seed)
        self.augment = _check_spec(augment, multi_view=False)
        if self.augment is not None and self.augment.crop_hw is not None:
            ch, cw = self.augment.crop_hw
            if ch < 1 or cw < 1 or ch > self.img_h or cw > self.img_w:
                raise ValueError(f"ScanNetFrames: a crop of {(ch, cw)} does not fit the resized image {(self.img_h, self.img_w)}")

    def __getitem__(self, i):
        from PIL import Image
        scene, sdir, idx = self._split(self.samples[i])
        aug = Augment() if self.augment is None else draw_augment(self.augment, *augment_rngs(self.seed, self.epoch, i), (self.img_h, self.img_w))
        with Image.open(self._color(sdir, idx)) as im, Image.open(self._depth(sdir, idx)) as dm:
            if self.raw_images:
                return {"img": torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)),
                        "depth": torch.from_numpy(np.array(dm, dtype=np.uint16)), "scene_name": scene, "img_idx": str(idx), "aug": aug}
            rgb = im.convert("RGB").resize((self.img_w, self.img_h), resample=Image.BILINEAR)
            dep = dm.resize((self.img_w, self.img_h), resample=Image.NEAREST)
            if aug.flip:
                rgb, dep = rgb.transpose(Image.FLIP_LEFT_RIGHT), dep.transpose(Image.FLIP_LEFT_RIGHT)
            img = np.array(rgb).astype(np.float32) / 255.0
            depth = self._depth_metres(np.array(dep))[:, :, None]
        if self.augment is not None and self.augment.crop_hw is not None:
            (x, y), (ch, cw) = aug.window, self.augment.crop_hw
            img, depth = img[y:y + ch, x:x + cw, :], depth[y:y + ch, x:x + cw, :]
        if aug.color is not None:
            img = augment_image(img, *aug.color)
        mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
        img = (torch.from_numpy(img).permute(2, 0, 1) - mean) / std
        return {"img": img, "depth": torch.from_numpy(np.ascontiguousarray(depth)).permute(2, 0, 1), "scene_name": scene, "img_idx": str(idx)}


class SevenScenesFrames(ScanNetFrames, SevenScenesFolder):
    """ScanNetFrames over the 7-Scenes layout: SevenScenesFolder's samples, file names and "no measurement" code."""


def collate_frames(items):
    """default_collate of ScanNetFrames items: tensors stacked (the raw uint8 frames and uint16 depth maps of one batch must share one
    raw size each), names and draws as lists."""
    for key in ("img", "depth"):
        sizes = {tuple(it[key].shape) for it in items}
        if len(sizes) > 1:
            raise ValueError("collate_frames: the %s entries of one batch have shapes %s; batch scenes of one raw size together" % (key, sorted(sizes)))
    out = {"img": torch.stack([it["img"] for it in items]), "depth": torch.stack([it["depth"] for it in items]),
           "scene_name": [it["scene_name"] for it in items], "img_idx": [it["img_idx"] for it in items]}
    if "aug" in items[0]:
        out["aug"] = [it["aug"] for it in items]
    return out


def collate(items):
    """What torch's default_collate makes of a list of (data_array, cam_intrins): per-frame dicts with a leading batch
    dimension ('extM' becomes a (B,4,4) float64 tensor), intrinsics stacked to (B,3,3) / (B,3,hw).  The uint8 frames of
    `raw_images=True` items stack to (B,Hraw,Wraw,3); one batch holds one raw size.  Of an augmenting raw folder, 'aug' becomes the
    list of the B draws and the reference frame's 'gt_dmap_raw' stacks to (B,Hd,Wd) uint16 (one depth size per batch); that dict
    has no 'gt_dmap' until ingest.prepare_train_batch makes it.  A list of ScanNetFrames items goes to collate_frames."""
    if isinstance(items[0], dict):
        return collate_frames(items)
    n_frames = len(items[0][0])
    raw_sizes = {tuple(d["img"].shape[:2]) for it in items for d in it[0] if d["img"].dtype == torch.uint8}
    if len(raw_sizes) > 1:
        raise ValueError("collate: the raw frames of one batch have sizes %s; batch scenes of one raw size together (or use batch size 1)"
                         % sorted(raw_sizes))
    data_array = []
    for f in range(n_frames):
        ds = [it[0][f] for it in items]
        entry = {"img": torch.stack([d["img"] for d in ds])}
        if "gt_dmap_raw" in ds[0]:
            if len({tuple(d["gt_dmap_raw"].shape) for d in ds}) > 1:
                raise ValueError("collate: the raw depth maps of one batch have sizes %s; batch scenes of one raw size together"
                                 % sorted({tuple(d["gt_dmap_raw"].shape) for d in ds}))
            entry["gt_dmap_raw"] = torch.stack([d["gt_dmap_raw"] for d in ds])
        else:
            gt = ds[0]["gt_dmap"]
            entry["gt_dmap"] = torch.stack([d["gt_dmap"] for d in ds]) if torch.is_tensor(gt) else torch.zeros(len(ds), dtype=torch.float64)
        entry.update({"extM": torch.from_numpy(np.stack([d["extM"] for d in ds])),
                      "scene_name": [d["scene_name"] for d in ds], "img_idx": [d["img_idx"] for d in ds]})
        if "aug" in ds[0]:
            entry["aug"] = [d["aug"] for d in ds]
        data_array.append(entry)
    intr = {k: torch.stack([it[1][k] for it in items]) for k in items[0][1]}
    return data_array, intr


def batches(dataset, batch_size=1):
    """Sequential batches of (data_array, cam_intrins), the iteration protocol of the reference's test loaders."""
    for s in range(0, len(dataset), batch_size):
        yield collate([dataset[i] for i in range(s, min(s + batch_size, len(dataset)))])
