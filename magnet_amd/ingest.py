"""Camera frames to the backbones' input on the device: crop, Pillow's 8-bit BILINEAR resize and the loader's normalisation in one
launch (lib.image_prep_u8, csrc/image_prep.hip), bit-identical to what `data.ScanNetFolder` computes on the host.

    prep = ImagePrep(raw_hw=(968, 1296), out_hw=(480, 640))
    imgs = prep.prep(frames_u8)              # (N, 968, 1296, 3) uint8, on the GPU or the host -> (N, 3, 480, 640) fp32 on the GPU

Why equality holds.  `Image.resize(size, resample=Image.BILINEAR)` on an 8-bit image is two integer passes (horizontal, then
vertical over the horizontal pass's uint8 result): out = clip8((2^21 + sum_k coef[k] * pixel[xmin + k]) >> 22) with int32
coefficients that Pillow derives in double precision from the two sizes alone.  `resample_tables` restates that derivation
(Pillow's precompute_coeffs / normalize_coeffs_8bpc, src/libImaging/Resample.c) operation for operation on the host, and the
kernel does the integer passes.  The normalisation `(x / 255 - mean) / std` sees only 256 inputs per channel: `normalise_table`
evaluates the loader's own expressions on all of them and the kernel looks the result up, so no floating-point operation of the
device, and no compiler flag, has a say in the output.

There is no CPU fallback and no approximate mode: a downscale ratio beyond the kernel's IMAGE_PREP_KMAX taps per axis raises."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import lib
from .data import IMAGENET_MEAN, IMAGENET_STD
from .lib import MagnetError

PRECISION_BITS = 32 - 8 - 2                                      # Pillow's fixed-point scale of an 8-bit coefficient


def resample_tables(in_size, out_size):
    """Pillow's BILINEAR coefficient tables of one pass from `in_size` to `out_size` pixels:
    (coef (out_size, ksize) int32, bounds (out_size, 2) int32 rows of (xmin, n)).  Output pixel xx is
    clip8((2^21 + sum_{k < n} coef[xx, k] * pixel[xmin + k]) >> 22); the entries of a row behind its n taps are 0.
    float64 throughout, in Pillow's order of operations: the filter argument is multiplied by 1 / filterscale (not divided by
    filterscale), the weights are summed in index order and each is divided by the sum."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise MagnetError(f"resample_tables: sizes {in_size} -> {out_size} must be positive")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                                  # the triangle filter's support is 1
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)      # astype truncates towards zero, as the C cast does
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    k = np.arange(ksize, dtype=np.int64)[None, :]
    arg = np.abs(((k + xmin[:, None]) - center[:, None] + 0.5) * (1.0 / filterscale))
    w = np.where((arg < 1.0) & (k < n[:, None]), 1.0 - arg, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):                                       # index order; the zeros behind a row's taps add nothing
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    coef = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)      # the weights are never negative: truncation rounds half up
    return coef, np.stack([xmin, n], axis=1).astype(np.int32)


def normalise_table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(3, 256) fp32: entry [c, v] is what data.ScanNetFolder makes of byte value v in channel c, by its very expressions (numpy fp32
    `/ 255.0`, then torch `(x - mean) / std`) on an image that holds every byte value once."""
    v = np.arange(256, dtype=np.uint8)
    rgb = np.stack([v, v, v], axis=-1)[None]                     # (1, 256, 3): one row, all three channels equal
    mean_t = torch.tensor(mean).view(3, 1, 1); std_t = torch.tensor(std).view(3, 1, 1)
    img = torch.from_numpy(rgb.astype(np.float32) / 255.0).permute(2, 0, 1)
    img = (img - mean_t) / std_t
    return img.reshape(3, 256).contiguous()


def taps(in_size, out_size):
    """Coefficients per output pixel of a pass (Pillow's ksize); 0 for a pass that is skipped."""
    in_size, out_size = int(in_size), int(out_size)
    return 0 if in_size == out_size else int(math.ceil(max(in_size / out_size, 1.0))) * 2 + 1


class ImagePrep:
    """uint8 frames of one raw size -> (N, 3, Hout, Wout) fp32 on `device`, what the folder loaders' host path produces for the same
    pixels.  raw_hw = (Hin, Win); out_hw = (Hout, Wout); crop = (left, top, width, height) inside the frame, applied first as
    im.crop((left, top, left + width, top + height)) would be (None: the whole frame).  The tables depend on the sizes alone; they are
    built here and uploaded once, by the first prep().  `frames_prepared` / `launches` count what prep() has done."""

    def __init__(self, raw_hw, out_hw, crop=None, device="cuda", mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.raw_hw = (int(raw_hw[0]), int(raw_hw[1]))
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        Hin, Win = self.raw_hw
        Hout, Wout = self.out_hw
        if min(Hin, Win, Hout, Wout) < 1:
            raise MagnetError(f"ImagePrep: raw size {self.raw_hw} and output size {self.out_hw} must be positive")
        self.crop = (0, 0, Win, Hin) if crop is None else tuple(int(v) for v in crop)
        if len(self.crop) != 4:
            raise MagnetError(f"ImagePrep: crop must be (left, top, width, height), got {crop!r}")
        left, top, cw, ch = self.crop
        if left < 0 or top < 0 or cw < 1 or ch < 1 or left + cw > Win or top + ch > Hin:
            raise MagnetError(f"ImagePrep: crop box left={left} top={top} {cw} x {ch} is not inside the {Win} x {Hin} frame")
        for name, n_in, n_out in (("horizontal", cw, Wout), ("vertical", ch, Hout)):
            if taps(n_in, n_out) > lib.IMAGE_PREP_KMAX:
                raise MagnetError(f"ImagePrep: the {name} pass {n_in} -> {n_out} needs {taps(n_in, n_out)} taps; the kernel's limit is "
                                  f"IMAGE_PREP_KMAX = {lib.IMAGE_PREP_KMAX} per axis (downscale ratios up to {(lib.IMAGE_PREP_KMAX - 1) // 2}); "
                                  "there is no CPU fallback", code=lib.E_SHAPE)
        self.device = torch.device(device)
        self._host = {"x": resample_tables(cw, Wout) if cw != Wout else None, "y": resample_tables(ch, Hout) if ch != Hout else None,
                      "lut": normalise_table(mean, std)}
        self._dev = None
        self.frames_prepared = 0
        self.launches = 0

    @classmethod
    def kitti(cls, raw_hw, device="cuda", img_hw=(352, 1216)):
        """The KITTI benchmark crop (dataloader_kitti.py:160-165): the bottom-centre 352 x 1216 box of the raw frame, no resize."""
        Hraw, Wraw = int(raw_hw[0]), int(raw_hw[1])
        top, left = int(Hraw - img_hw[0]), int((Wraw - img_hw[1]) / 2)
        return cls(raw_hw, img_hw, crop=(left, top, img_hw[1], img_hw[0]), device=device)

    def tables(self):
        """The device tables (tables_x, tables_y, lut), uploaded on first use."""
        if self._dev is None:
            up = lambda t: None if t is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in t)
            self._dev = (up(self._host["x"]), up(self._host["y"]), self._host["lut"].to(self.device))
        return self._dev

    def check(self, frames_u8):
        """Raises MagnetError unless `frames_u8` is a uint8 (N, Hin, Win, 3) tensor of this prep's raw size."""
        f = frames_u8
        if not isinstance(f, torch.Tensor):
            raise MagnetError(f"ImagePrep: expected a torch.Tensor of frames, got {type(f).__name__}")
        if f.dtype != torch.uint8:
            raise MagnetError(f"ImagePrep: frames must be uint8 (decoded pixels, not normalised), got {f.dtype}")
        if f.dim() != 4 or f.shape[3] != 3 or f.shape[0] < 1:
            raise MagnetError(f"ImagePrep: frames must be (N, Hin, Win, 3) channel-last with N >= 1, got {tuple(f.shape)}")
        if tuple(f.shape[1:3]) != self.raw_hw:
            raise MagnetError(f"ImagePrep: frames of raw size {tuple(f.shape[1:3])}, this prep was built for {self.raw_hw}")

    def prep(self, frames_u8, out=None):
        """frames_u8: uint8 (N, Hin, Win, 3) on this prep's GPU, or on the host (uploaded as uint8; without blocking if pinned).
        Returns (N, 3, Hout, Wout) fp32 on the device: `out` if given, else a new tensor.  One launch."""
        self.check(frames_u8)
        f = frames_u8
        N = int(f.shape[0])
        shape = (N, 3) + self.out_hw
        if out is not None:
            if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
                raise MagnetError(f"ImagePrep: out must be a contiguous fp32 tensor of shape {shape}, got "
                                  f"{tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__}")
            if out.device != self.device and not (out.is_cuda and self.device.index is None):
                raise MagnetError(f"ImagePrep: out is on {out.device}, this prep works on {self.device}")
        if not f.is_cuda:
            f = f.to(self.device if out is None else out.device, non_blocking=f.is_pinned())
        elif self.device.index is not None and f.device != self.device:
            raise MagnetError(f"ImagePrep: frames are on {f.device}, this prep works on {self.device}")
        if f.stride(3) != 1 or f.stride(2) != 3 or f.stride(1) < 3 * f.shape[2] or (N > 1 and f.stride(0) < f.stride(1) * f.shape[1]):
            f = f.contiguous()                                   # rows and frames may carry a pitch; anything else is copied once
        if self.device.index is None:
            self.device = f.device                               # "cuda" meant the current device: it is this one from now on
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=f.device)
        tx, ty, lut = self.tables()
        lib.image_prep_u8(f, out, self.crop, tx, ty, lut)
        self.frames_prepared += N
        self.launches += 1
        return out


class ImagePrepSet:
    """One ImagePrep per raw size, built when frames of that size first arrive: what a dataset whose scenes differ in resolution
    needs.  prep() and check() as ImagePrep's; `crop` is None or a function raw_hw -> (left, top, width, height)."""

    def __init__(self, out_hw, crop=None, device="cuda"):
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.crop, self.device = crop, device
        self.preps = {}

    def _for(self, frames_u8):
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4:
            raise MagnetError("ImagePrep: frames must be a uint8 (N, Hin, Win, 3) tensor")
        raw_hw = (int(frames_u8.shape[1]), int(frames_u8.shape[2]))
        if raw_hw not in self.preps:
            self.preps[raw_hw] = ImagePrep(raw_hw, self.out_hw, None if self.crop is None else self.crop(raw_hw), self.device)
        return self.preps[raw_hw]

    def check(self, frames_u8):
        self._for(frames_u8).check(frames_u8)

    def prep(self, frames_u8, out=None):
        return self._for(frames_u8).prep(frames_u8, out)

    @property
    def frames_prepared(self):
        return sum(p.frames_prepared for p in self.preps.values())

    @property
    def launches(self):
        return sum(p.launches for p in self.preps.values())


# ---- what the evaluation drivers share (--device_images) ----
class DeviceImages:
    """A loader of `raw_images=True` batches with every 'img' prepared on the device: the uint8 frames of a batch (all entries of a
    window batch's data_array, or a single-view batch dict) go up as uint8 and through ONE launch; each 'img' becomes its
    (B, 3, H, W) fp32 slice of the result, on the device, so a driver's `.to(device)` has nothing left to do.  Everything else of a
    batch passes through untouched."""

    def __init__(self, loader, preps):
        self.loader, self.preps = loader, preps

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield prepare_batch(batch, self.preps)


def prepare_batch(batch, preps):
    """`batch`: (data_array, cam_intrins) or one dict with 'img'.  Returns the same structure with the uint8 'img' entries replaced."""
    single = isinstance(batch, dict)
    dicts = [batch] if single else list(batch[0])
    imgs = [d["img"] for d in dicts]
    if len({tuple(t.shape[1:]) for t in imgs}) != 1:
        raise MagnetError(f"device images: the frames of one batch have raw sizes {sorted({tuple(t.shape[1:3]) for t in imgs})}: one batch, one raw size")
    out = preps.prep(imgs[0] if len(imgs) == 1 else torch.cat(imgs, dim=0))
    new, first = [], 0
    for d, t in zip(dicts, imgs):
        new.append({**d, "img": out[first:first + t.shape[0]]})
        first += t.shape[0]
    return new[0] if single else (new, batch[1])


def add_arguments(ap):
    ap.add_argument("--device_images", action="store_true",
                    help="with --dataset_path: the loader hands out the decoded uint8 frames (raw_images=True) and crop / resize / normalisation "
                         "run on the device (magnet_amd/ingest.py), bit-identical to the host path: the metrics do not change")


def device_image_loader(a, loader, device, to_runner=False):
    """The driver side of --device_images for a loader over a `raw_images=True` folder: -> (loader, preps).  preps: an ImagePrepSet for
    (a.input_height, a.input_width).  to_runner: the frames stay uint8 in the batches, for a SequenceRunner(image_prep=preps), which
    prepares only the frames its pool lacks; otherwise the loader is wrapped in DeviceImages."""
    preps = ImagePrepSet((a.input_height, a.input_width), device=device)
    return (loader if to_runner else DeviceImages(loader, preps)), preps
