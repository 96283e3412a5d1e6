"""The yardstick of the training-sample preparation: Pillow and numpy evaluating the reference loaders' expressions on whole images
(data/dataloader_scannet.py:171-200,219-232, dataloader_scannet_D.py:80-156, dataloader_kitti_D.py:80-160), restated once, here.
Nothing of magnet_amd is used: neither its tables nor its host path."""
import numpy as np
import torch
from PIL import Image

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def colour(image, gamma, brightness, colors):
    """(H, W, 3) float32 in [0, 1] -> the loaders' augment_image: float32 power and product, the in-place product with a float64
    colour image, the clip."""
    out = image ** gamma
    out = out * brightness
    white = np.ones((image.shape[0], image.shape[1]))
    out *= np.stack([white * colors[0], white * colors[1], white * colors[2]], axis=2)
    return np.clip(out, 0, 1)


def normalise(img_hwc):
    """(H, W, 3) float32 -> (3, H, W): torchvision's Normalize as the loaders call it, (x - mean) / std in fp32."""
    t = torch.from_numpy(np.ascontiguousarray(img_hwc)).permute(2, 0, 1)
    return (t - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


def box_of(crop):
    left, top, w, h = crop
    return (left, top, left + w, top + h)


def image(frame_u8, res_hw, out_hw, crop=None, color=None, flip=False, window=(0, 0)):
    """(Hin, Win, 3) uint8 -> (3, Hout, Wout) fp32 tensor: crop box, BILINEAR resize to res_hw, flip, / 255, window, colour, normalise."""
    im = Image.fromarray(frame_u8)
    if crop is not None:
        im = im.crop(box_of(crop))
    if (im.height, im.width) != tuple(res_hw):
        im = im.resize((res_hw[1], res_hw[0]), resample=Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    img = np.array(im).astype(np.float32) / 255.0
    x, y = window
    img = img[y:y + out_hw[0], x:x + out_hw[1], :]
    assert img.shape[:2] == tuple(out_hw)
    if color is not None:
        img = colour(img, *color)
    return normalise(img)


def depth(depth_u16, res_hw, out_hw, crop=None, flip=False, window=(0, 0), divisor=1000.0, invalid=None):
    """(Hin, Win) uint16 -> (1, Hout, Wout) fp32 tensor: crop box, NEAREST resize, flip, invalid code -> 0, float32 / divisor, window."""
    im = Image.fromarray(depth_u16)
    assert im.mode == "I;16"
    if crop is not None:
        im = im.crop(box_of(crop))
    if (im.height, im.width) != tuple(res_hw):
        im = im.resize((res_hw[1], res_hw[0]), resample=Image.NEAREST)
    d = np.array(im)
    assert d.dtype == np.uint16
    if flip:
        d = d[:, ::-1]
    d = d.copy()
    if invalid is not None:
        d[d == invalid] = 0
    d = d[:, :, np.newaxis].astype(np.float32)
    d = d / divisor
    x, y = window
    d = d[y:y + out_hw[0], x:x + out_hw[1], :]
    assert d.shape[:2] == tuple(out_hw)
    return torch.from_numpy(np.ascontiguousarray(d)).permute(2, 0, 1)


def bits(t):
    """The 32 bits of every fp32 element, for comparisons that tell -0.0 from 0.0 and NaN from NaN."""
    return t.contiguous().view(torch.int32)


# ---- what the host and the GPU tests share: draws that include the ends of the ranges and a product that clips ----
COLOURS = [(0.9, 0.75, (0.9, 0.9, 0.9)), (1.1, 1.25, (1.1, 1.1, 1.1)), (0.9, 1.25, (1.1, 0.9, 1.1)), (1.1, 0.75, (0.9, 1.1, 1.0)),
           (1.0, 1.0, (1.0, 1.0, 1.0))]


def seeded_colours(n, seed=0):
    import random
    py, nr = random.Random(seed), np.random.RandomState(seed)
    return [(py.uniform(0.9, 1.1), py.uniform(0.75, 1.25), tuple(float(c) for c in nr.uniform(0.9, 1.1, size=3))) for _ in range(n)]
