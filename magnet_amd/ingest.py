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

There is no CPU fallback and no approximate mode: a downscale ratio beyond the kernel's IMAGE_PREP_KMAX taps per axis raises.

Training samples (TrainPrep; lib.train_prep_u8, lib.depth_prep_u16) extend the same argument.  After the resize the image is still 8
bits per channel, and flip and crop window only move pixels, so everything the training loaders compute on the image side (`/ 255`,
`clip(x ** gamma * brightness * colour_c, 0, 1)`, the normalisation) is a function of (byte value, channel, the sample's draw):
`augment_table` evaluates the loader's own expressions on all 256 values and the kernel looks them up, one table per augmented
sample.  The ground-truth depth is Pillow's NEAREST resize, an index table per axis (`nearest_table`), a compare and one correctly
rounded fp32 division.  Equal to `data.ScanNetFolder(augment=...)` / `data.ScanNetFrames` on the host, bit for bit."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import lib
from .data import IMAGENET_MEAN, IMAGENET_STD, Augment, augment_image
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


def nearest_table(in_size, out_size):
    """(out_size,) int32: the source index Pillow's NEAREST resize from `in_size` to `out_size` pixels reads for every output pixel,
    floor((x + 0.5) * (in_size / out_size)) in float64 (the per-pixel form; accumulating `+= scale` differs, e.g. at 1000 -> 333).
    tests/test_train_prep_host.py holds it against the installed Pillow on I;16 ramps."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise MagnetError(f"nearest_table: sizes {in_size} -> {out_size} must be positive")
    idx = np.floor((np.arange(out_size, dtype=np.float64) + 0.5) * (in_size / out_size)).astype(np.int64)
    return np.minimum(idx, in_size - 1).astype(np.int32)


def augment_table(color=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(3, 256) fp32: entry [c, v] is what a training loader makes of byte value v in channel c under the draw
    color = (gamma, brightness, colors[3]): numpy fp32 `/ 255.0`, data.augment_image (the expressions of dataloader_scannet.py:219-232
    with their dtypes: fp32 power and product, the in-place product with the float64 colour image, the clip), then torch
    `(x - mean) / std`, on an image that holds every byte value once.  color None: exactly normalise_table()."""
    if color is None:
        return normalise_table(mean, std)
    gamma, brightness, colors = color
    v = np.arange(256, dtype=np.uint8)
    img = np.stack([v, v, v], axis=-1)[None].astype(np.float32) / 255.0      # (1, 256, 3)
    img = augment_image(img, gamma, brightness, colors)
    mean_t = torch.tensor(mean).view(3, 1, 1); std_t = torch.tensor(std).view(3, 1, 1)
    img = (torch.from_numpy(img).permute(2, 0, 1) - mean_t) / std_t
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


# ---- training samples ----
class TrainParams:
    """What one upload of TrainPrep.params() left on the device: `luts` (L, 3, 256) fp32 and `records` (N, 4) int32 rows of
    (lut_index, flip, win_x, win_y).  p[i:j] is the same upload seen by the frames i..j-1 (the reference frames' depth maps)."""

    def __init__(self, luts, records):
        self.luts, self.records = luts, records

    def __len__(self):
        return int(self.records.shape[0])

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise MagnetError("TrainParams: only contiguous slices p[i:j] share an upload")
        return TrainParams(self.luts, self.records[s])


class TrainPrep:
    """Training samples of one raw size on `device`, what data.ScanNetFolder(augment=...) / data.ScanNetFrames compute on the host,
    to the bit.  raw_hw = (Hin, Win) of the colour frames; crop = (left, top, width, height) as ImagePrep's; resize_hw = (Hres, Wres):
    Pillow's resize of the crop box (BILINEAR for the frames, NEAREST for the depth); out_hw = (Hout, Wout): the crop window every
    Augment places inside the (flipped) resized image (None: all of it).  depth_divisor 1000 (ScanNet, 7-Scenes) or 256 (KITTI);
    depth_invalid: the sensor's "no measurement" code that becomes 0 (7-Scenes: 65535), or None.

        p = prep.params(augs)                   # ONE host-to-device copy: the tables of the batch's colour draws + an (N, 4) record
        imgs = prep.prep(frames_u8, p)          # (N, Hin, Win, 3) uint8 -> (N, 3, Hout, Wout) fp32, one launch
        gt = prep.prep_depth(depth_u16, p)      # (N, Hd, Wd) uint16 -> (N, 1, Hout, Wout) fp32, one launch

    prep / prep_depth also take the sequence of Augments itself (and then upload it).  Depth maps may have another raw size than the
    frames (ScanNet: 640 x 480 against 1296 x 968) when there is no crop box; their index tables are built per size.  Every window is
    checked here on the host.  `uploads`, `launches`, `frames_prepared`, `depths_prepared` count what has been done."""

    def __init__(self, raw_hw, resize_hw, out_hw=None, crop=None, depth_divisor=1000.0, depth_invalid=None, device="cuda",
                 mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.images = ImagePrep(raw_hw, resize_hw, crop=crop, device=device, mean=mean, std=std)       # sizes, crop box, taps: checked there
        self.raw_hw, self.resize_hw, self.has_crop = self.images.raw_hw, self.images.out_hw, crop is not None
        self.out_hw = self.resize_hw if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        if not (1 <= self.out_hw[0] <= self.resize_hw[0] and 1 <= self.out_hw[1] <= self.resize_hw[1]):
            raise MagnetError(f"TrainPrep: a crop window of {self.out_hw} does not fit the resized image {self.resize_hw}")
        self.depth_divisor = float(depth_divisor)
        if not (math.isfinite(self.depth_divisor) and self.depth_divisor > 0.0):
            raise MagnetError(f"TrainPrep: depth_divisor {depth_divisor} must be finite and positive")
        self.depth_invalid = -1 if depth_invalid is None else int(depth_invalid)
        self.mean, self.std = mean, std
        self._depth_tables = {}
        self.uploads = self.launches = self.frames_prepared = self.depths_prepared = 0

    @classmethod
    def kitti(cls, raw_hw, out_hw=None, device="cuda", img_hw=(352, 1216)):
        """The KITTI benchmark crop (dataloader_kitti_D.py:80-87) of frame and depth, no resize, depth / 256."""
        box = ImagePrep.kitti(raw_hw, device=device, img_hw=img_hw).crop
        return cls(raw_hw, img_hw, out_hw=out_hw, crop=box, depth_divisor=256.0, device=device)

    @property
    def device(self):
        return self.images.device

    def records(self, augs):
        """The host side of params(): (tables (L, 3, 256) fp32 with table 0 the plain normalisation and one more per distinct colour
        draw, records (N, 4) int32).  Raises MagnetError for anything but Augments whose windows lie inside the resized image."""
        (Hres, Wres), (Hout, Wout) = self.resize_hw, self.out_hw
        tables, index, rec = [self.images._host["lut"]], {None: 0}, []
        for n, a in enumerate(augs):
            if not isinstance(a, Augment):
                raise MagnetError(f"TrainPrep: augs[{n}] is a {type(a).__name__}, expected a magnet_amd.data.Augment")
            x, y = (0, 0) if a.window is None else (int(a.window[0]), int(a.window[1]))
            if x < 0 or y < 0 or x + Wout > Wres or y + Hout > Hres:
                raise MagnetError(f"TrainPrep: augs[{n}]: the {Hout} x {Wout} window at x={x} y={y} is not inside the resized {Hres} x {Wres} image")
            key = None if a.color is None else (float(a.color[0]), float(a.color[1]), tuple(float(c) for c in a.color[2]))
            if key not in index:
                index[key] = len(tables)
                tables.append(augment_table(key, self.mean, self.std))
            rec.append((index[key], int(bool(a.flip)), x, y))
        if not rec:
            raise MagnetError("TrainPrep: no Augment given; a batch has one per frame")
        return torch.stack(tables), torch.tensor(rec, dtype=torch.int32)

    def params(self, augs):
        """Uploads the tables and records of `augs` (one Augment per frame) in ONE host-to-device copy from a pinned staging
        buffer -> TrainParams."""
        if isinstance(augs, TrainParams):
            return augs
        luts, rec = self.records(augs)
        n_lut = luts.numel() * 4
        stage = torch.empty(n_lut + rec.numel() * 4, dtype=torch.uint8, pin_memory=True)
        stage[:n_lut].view(torch.float32).copy_(luts.reshape(-1))
        stage[n_lut:].view(torch.int32).copy_(rec.reshape(-1))
        dev = stage.to(self.device, non_blocking=True)
        self.uploads += 1
        return TrainParams(dev[:n_lut].view(torch.float32).view(-1, 3, 256), dev[n_lut:].view(torch.int32).view(-1, 4))

    def _src(self, t, out, name):
        if not t.is_cuda:
            return t.to(self.device if out is None else out.device, non_blocking=t.is_pinned())
        if self.device.index is not None and t.device != self.device:
            raise MagnetError(f"TrainPrep: {name} are on {t.device}, this prep works on {self.device}")
        return t

    def _out(self, out, shape, src):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=src.device)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise MagnetError(f"TrainPrep: out must be a contiguous fp32 tensor of shape {shape}, got "
                              f"{tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__}")
        if out.device != src.device:
            raise MagnetError(f"TrainPrep: out is on {out.device}, the frames on {src.device}")
        return out

    def _params_for(self, augs, N):
        n = len(augs)
        if n != N:
            raise MagnetError(f"TrainPrep: {n} Augments for {N} frames: a batch has one per frame")
        return self.params(augs)

    def prep(self, frames_u8, augs, out=None):
        """frames_u8: uint8 (N, Hin, Win, 3) on this prep's GPU or on the host; augs: N Augments or a TrainParams of N records.
        Returns (N, 3, Hout, Wout) fp32 on the device.  One launch."""
        self.images.check(frames_u8)
        N = int(frames_u8.shape[0])
        p = self._params_for(augs, N)
        f = self._src(frames_u8, out, "frames")
        if f.stride(3) != 1 or f.stride(2) != 3 or f.stride(1) < 3 * f.shape[2] or (N > 1 and f.stride(0) < f.stride(1) * f.shape[1]):
            f = f.contiguous()
        if self.images.device.index is None:
            self.images.device = f.device
        out = self._out(out, (N, 3) + self.out_hw, f)
        tx, ty, _ = self.images.tables()
        lib.train_prep_u8(f, out, self.images.crop, self.resize_hw, tx, ty, p.luts, p.records)
        self.frames_prepared += N
        self.launches += 1
        return out

    def depth_tables(self, depth_hw):
        """(crop box, idx_x, idx_y) for depth maps of raw size `depth_hw`; the device tables are uploaded on first use."""
        depth_hw = (int(depth_hw[0]), int(depth_hw[1]))
        if depth_hw not in self._depth_tables:
            if self.has_crop and depth_hw != self.raw_hw:
                raise MagnetError(f"TrainPrep: depth maps of raw size {depth_hw} with a crop box made for frames of {self.raw_hw}")
            box = self.images.crop if self.has_crop else (0, 0, depth_hw[1], depth_hw[0])
            up = lambda n_in, n_out: None if n_in == n_out else torch.from_numpy(nearest_table(n_in, n_out)).to(self.device)
            self._depth_tables[depth_hw] = (box, up(box[2], self.resize_hw[1]), up(box[3], self.resize_hw[0]))
        return self._depth_tables[depth_hw]

    def prep_depth(self, depth_u16, augs, out=None):
        """depth_u16: uint16 (N, Hd, Wd) on this prep's GPU or on the host; augs as prep()'s.  Returns (N, 1, Hout, Wout) fp32 on the
        device: NEAREST resize, flip, window, depth_invalid -> 0, / depth_divisor.  One launch."""
        d = depth_u16
        if not isinstance(d, torch.Tensor):
            raise MagnetError(f"TrainPrep: expected a torch.Tensor of depth maps, got {type(d).__name__}")
        if d.dtype != torch.uint16:
            raise MagnetError(f"TrainPrep: depth maps must be uint16 (the decoded PNG, not metres), got {d.dtype}")
        if d.dim() != 3 or d.shape[0] < 1:
            raise MagnetError(f"TrainPrep: depth maps must be (N, Hd, Wd) with N >= 1, got {tuple(d.shape)}")
        N = int(d.shape[0])
        p = self._params_for(augs, N)
        d = self._src(d, out, "depth maps")
        if d.stride(2) != 1 or d.stride(1) < d.shape[2] or (N > 1 and d.stride(0) < d.stride(1) * d.shape[1]):
            d = d.contiguous()
        if self.images.device.index is None:
            self.images.device = d.device
        out = self._out(out, (N, 1) + self.out_hw, d)
        box, ix, iy = self.depth_tables(d.shape[1:])
        lib.depth_prep_u16(d, out, box, self.resize_hw, ix, iy, p.records, self.depth_divisor, self.depth_invalid)
        self.depths_prepared += N
        self.launches += 1
        return out


class TrainPrepSet:
    """One TrainPrep per raw frame size, built when frames of that size first arrive; mirrors ImagePrepSet.  `crop` is None or a function
    raw_hw -> (left, top, width, height).  params / prep / prep_depth take the frames' raw size from `frames_u8`; prep_depth, which
    sees no frame, takes it as `raw_hw`."""

    def __init__(self, resize_hw, out_hw=None, crop=None, depth_divisor=1000.0, depth_invalid=None, device="cuda"):
        self.resize_hw, self.out_hw, self.crop = resize_hw, out_hw, crop
        self.kw = dict(depth_divisor=depth_divisor, depth_invalid=depth_invalid, device=device)
        self.preps = {}

    def for_raw(self, raw_hw):
        raw_hw = (int(raw_hw[0]), int(raw_hw[1]))
        if raw_hw not in self.preps:
            self.preps[raw_hw] = TrainPrep(raw_hw, self.resize_hw, self.out_hw, None if self.crop is None else self.crop(raw_hw), **self.kw)
        return self.preps[raw_hw]

    def _for(self, frames_u8):
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4:
            raise MagnetError("TrainPrep: frames must be a uint8 (N, Hin, Win, 3) tensor")
        return self.for_raw(frames_u8.shape[1:3])

    def params(self, frames_u8, augs):
        return self._for(frames_u8).params(augs)

    def prep(self, frames_u8, augs, out=None):
        return self._for(frames_u8).prep(frames_u8, augs, out)

    def prep_depth(self, depth_u16, augs, raw_hw, out=None):
        return self.for_raw(raw_hw).prep_depth(depth_u16, augs, out)

    def _sum(self, name):
        return sum(getattr(p, name) for p in self.preps.values())

    uploads = property(lambda self: self._sum("uploads"))
    launches = property(lambda self: self._sum("launches"))
    frames_prepared = property(lambda self: self._sum("frames_prepared"))
    depths_prepared = property(lambda self: self._sum("depths_prepared"))


class DeviceTrainBatches:
    """A loader of collated `raw_images=True, augment=...` batches with every sample prepared on the device (prepare_train_batch): one
    upload of tables and records, one launch for all frames, one for the depth maps."""

    def __init__(self, loader, preps):
        self.loader, self.preps = loader, preps

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield prepare_train_batch(batch, self.preps)


def prepare_train_batch(batch, preps):
    """`batch`: the collated (data_array, cam_intrins) of a data.ScanNetFolder(raw_images=True, augment=...), or the collated dict of a
    data.ScanNetFrames(raw_images=True).  `preps`: a TrainPrep or TrainPrepSet.  Returns the structure the host path hands out, on
    the device: every uint8 'img' becomes its (B, 3, H, W) fp32 tensor, the uint16 'gt_dmap_raw' becomes 'gt_dmap' (B, 1, H, W) and the
    uint16 'depth' becomes (B, 1, H, W) fp32; 'aug' is dropped; everything else passes through."""
    single = isinstance(batch, dict)
    dicts = [batch] if single else list(batch[0])
    imgs = [d["img"] for d in dicts]
    if len({tuple(t.shape[1:]) for t in imgs}) != 1:
        raise MagnetError(f"device training batches: the frames of one batch have raw sizes {sorted({tuple(t.shape[1:3]) for t in imgs})}: one batch, one raw size")
    if any("aug" not in d for d in dicts):
        raise MagnetError("device training batches: a batch without 'aug' entries; build the folder with raw_images=True and an AugmentSpec")
    frames = imgs[0] if len(imgs) == 1 else torch.cat(imgs, dim=0)
    prep = preps.for_raw(frames.shape[1:3]) if isinstance(preps, TrainPrepSet) else preps
    params = prep.params([a for d in dicts for a in d["aug"]])
    out = prep.prep(frames, params)
    new, first = [], 0
    for d, t in zip(dicts, imgs):
        B = int(t.shape[0])
        e = {k: v for k, v in d.items() if k not in ("aug", "gt_dmap_raw")}
        e["img"] = out[first:first + B]
        if "gt_dmap_raw" in d:
            e["gt_dmap"] = prep.prep_depth(d["gt_dmap_raw"], params[first:first + B])
        elif single:
            e["depth"] = prep.prep_depth(d["depth"], params[first:first + B])
        new.append(e)
        first += B
    return new[0] if single else (new, batch[1])


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
