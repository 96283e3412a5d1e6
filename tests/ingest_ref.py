"""A plain numpy / Python restatement of what magnet_image_prep_u8 computes: im.crop(box), then Pillow's 8-bit
Image.resize(size, resample=BILINEAR) (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal pass, then
the vertical pass over its uint8 result; a pass whose size does not change is skipped), then the loader's normalisation as a lookup.
Written with scalar loops for the tables, independently of magnet_amd.ingest.resample_tables; tests/test_ingest_host.py holds it
against Pillow itself byte for byte, and against the loader's expressions."""
import math

import numpy as np

BITS = 22

# ---- what the host and the GPU tests share ----
OUT_HW = (48, 64)
# raw (H, W): 7 taps with windows clipped at both borders; upscale, 3 taps; one pass skipped (twice); identity
RAW_HW = [(97, 131), (30, 40), (121, 64), (48, 200), (48, 64)]


def make_image(kind, hw, seed=0):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, hw + (3,), dtype=np.uint8)
    if kind == "binary":
        return (rng.randint(0, 2, hw + (3,)) * 255).astype(np.uint8)
    return np.full(hw + (3,), {"ones": 255, "zeros": 0}[kind], dtype=np.uint8)


def tables(in_size, out_size):
    """-> (coef [out][ksize] int, bounds [out] of (xmin, n)) of one BILINEAR pass, in double precision, Pillow's order of operations."""
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale > 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    coef, bounds = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)                        # int() truncates towards zero, as the C cast does
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        ws, ww = [], 0.0
        for x in range(n):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            w = 1.0 - t if t < 1.0 else 0.0
            ws.append(w)
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        row = [int(0.5 + w * (1 << BITS)) for w in ws] + [0] * (ksize - n)
        coef.append(row)
        bounds.append((xmin, n))
    return coef, bounds


def resample_pass(img, out_size, axis):
    """One pass over a (H, W, 3) uint8 image along `axis` (1: horizontal, 0: vertical); the image itself when the size stays."""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    coef, bounds = tables(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)               # (in, other, 3)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        acc = np.full(src.shape[1:], 1 << (BITS - 1), dtype=np.int64)
        for k in range(n):
            acc += coef[xx][k] * src[xmin + k]
        assert int(acc.max()) < 2 ** 31 and int(acc.min()) >= 0     # the kernel's int32 accumulator holds it
        out[xx] = np.clip(acc >> BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, out_hw, crop=None):
    """(H, W, 3) uint8 -> (Hout, Wout, 3) uint8: crop = (left, top, width, height) first, then horizontal pass, then vertical pass."""
    if crop is not None:
        left, top, cw, ch = crop
        assert 0 <= left and 0 <= top and left + cw <= img.shape[1] and top + ch <= img.shape[0]
        img = img[top:top + ch, left:left + cw]
    return resample_pass(resample_pass(img, out_hw[1], 1), out_hw[0], 0)


def lookup(mean, std):
    """(3, 256) float32 by the loader's expressions (magnet_amd/data.py: numpy fp32 / 255.0, then torch (x - mean) / std), evaluated
    one value at a time."""
    import torch
    lut = np.empty((3, 256), dtype=np.float32)
    for c in range(3):
        for v in range(256):
            x = torch.from_numpy(np.asarray([[[v]]], dtype=np.uint8).astype(np.float32) / 255.0)
            lut[c, v] = float(((x - torch.tensor(mean[c])) / torch.tensor(std[c])).reshape(()))
    return lut


def image_prep(frames, out_hw, crop=None, mean=None, std=None):
    """(N, H, W, 3) uint8 -> (N, 3, Hout, Wout) float32: the expected output of ImagePrep.prep."""
    from magnet_amd.data import IMAGENET_MEAN, IMAGENET_STD
    lut = lookup(mean or IMAGENET_MEAN, std or IMAGENET_STD)
    out = np.empty((frames.shape[0], 3) + tuple(out_hw), dtype=np.float32)
    for i in range(frames.shape[0]):
        r = resize_u8(frames[i], out_hw, crop)
        for c in range(3):
            out[i, c] = lut[c][r[..., c]]
    return out
