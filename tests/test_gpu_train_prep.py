"""-m gpu: training samples prepared on the device (magnet_train_prep_u8, magnet_depth_prep_u16, magnet_amd/ingest.py: TrainPrep).
The yardstick is Pillow and numpy on whole images (tests/train_prep_ref.py); every comparison is on all 32 bits, zero mismatches.
Shapes are chosen against the kernel's 80 x 10 output tile; every launch has three frames with different records and tables, one of
them the identity record, and writes between two guard blocks that must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

from magnet_amd import data, ingest, lib
from magnet_amd.data import Augment
from tests import train_prep_ref as ref
from tests.test_data_loader import _make_scene

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 4096
C1, C2, C3 = ref.COLOURS[0], ref.COLOURS[2], ref.seeded_colours(1, seed=5)[0]

# name: raw (H, W), crop box (left, top, w, h) or None, resized (H, W), window (H, W), origins (x, y), source row pitch in pixels
GEOMETRIES = {
    "downscale": dict(raw=(61, 97), crop=None, res=(23, 41), out=(17, 29), origins=[(0, 0), (12, 6), (5, 3)], pitch=None),
    "upscale": dict(raw=(23, 41), crop=None, res=(61, 97), out=(61, 97), origins=[(0, 0)], pitch=None),            # two tile columns, Wres odd
    "no_resize": dict(raw=(40, 200), crop=(7, 3, 190, 36), res=(36, 190), out=(32, 176), origins=[(14, 4), (0, 0), (9, 2)], pitch=211),
    "tap_limit": dict(raw=(160, 720), crop=None, res=(20, 90), out=(11, 81), origins=[(9, 9), (0, 0), (4, 5)], pitch=None),   # 8x: 17 taps
}


def launches(g):
    """Two lists of three Augments per geometry: every origin flipped and not, the identity record in another place each time."""
    o = g["origins"]
    ident = Augment(None, False, (0, 0))
    first = [ident, Augment(C1, True, o[-1]), Augment(C2, False, o[1 % len(o)])]
    second = [Augment(C3, True, o[0]), Augment(C1, False, o[-1]), ident]
    if g["out"] == g["res"]:                                      # the full window: flipped twice, with two tables
        return [[Augment(C1, True, (0, 0)), ident, Augment(C2, True, None)]]
    return [first, second, [Augment(C2, True, o[1 % len(o)]), ident, Augment(None, True, o[0])]]


def guarded(shape, gpu):
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=gpu)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def with_pitch(t, pitch, gpu, fill):
    """The (N, H, W[, 3]) host tensor on the device with rows `pitch` pixels apart, the gap filled with `fill`."""
    N, H, W = t.shape[:3]
    wide = np.full((N, H, pitch) + tuple(t.shape[3:]), fill, dtype=t.numpy().dtype)          # built on the host: uint16 has few device operators
    wide[:, :, :W] = t.numpy()
    view = torch.from_numpy(wide).to(gpu)[:, :, :W]
    assert not view.is_contiguous()
    return view


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_train_prep_kernel_equals_pillow_and_numpy(hip_lib, gpu, name):
    g = GEOMETRIES[name]
    H, W = g["raw"]
    frames = np.random.RandomState(len(name)).randint(0, 256, (3, H, W, 3), dtype=np.uint8)
    frames[1, :, : W // 2] = 255                                  # a saturated half: the clip of the colour product
    prep = ingest.TrainPrep(g["raw"], g["res"], out_hw=g["out"], crop=g["crop"], device=gpu)
    src = torch.from_numpy(frames)
    src = src.to(gpu) if g["pitch"] is None else with_pitch(src, g["pitch"], gpu, 0xA5)
    for augs in launches(g):
        assert len({(a.color, a.flip, a.window) for a in augs}) == 3 and Augment(None, False, (0, 0)) in augs
        buf, out = guarded((3, 3) + g["out"], gpu)
        lib.entry_log = log = []
        try:
            assert prep.prep(src, augs, out=out) is out
        finally:
            lib.entry_log = None
        assert log == ["magnet_train_prep_u8"]                   # one launch for all three frames
        exp = torch.stack([ref.image(frames[n], g["res"], g["out"], g["crop"], a.color, a.flip, a.window or (0, 0)) for n, a in enumerate(augs)])
        got = out.cpu()
        mism = int((ref.bits(got) != ref.bits(exp)).sum())
        print(f"{name}: {mism} mismatches of {exp.numel()}")
        assert mism == 0 and guards_untouched(buf)
    assert prep.uploads == prep.launches == len(launches(g)) and prep.frames_prepared == 3 * len(launches(g))


def depth_maps(hw, seed):
    """Three uint16 maps: random values with every special one planted (0, 1, 999, 1000, 1001, 65534, 65535)."""
    rng = np.random.RandomState(seed)
    d = rng.randint(0, 65536, (3,) + hw).astype(np.uint16)
    special = np.array([0, 1, 999, 1000, 1001, 65534, 65535], dtype=np.uint16)
    d[:, ::3, ::2] = special[rng.randint(0, 7, d[:, ::3, ::2].shape)]
    return d


@pytest.mark.parametrize("divisor,invalid", [(1000.0, 65535), (256.0, None), (1000.0, None)])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_depth_prep_kernel_equals_pillow_and_numpy(hip_lib, gpu, name, divisor, invalid):
    g = GEOMETRIES[name]
    maps = depth_maps(g["raw"], seed=len(name) + 1)
    prep = ingest.TrainPrep(g["raw"], g["res"], out_hw=g["out"], crop=g["crop"], depth_divisor=divisor, depth_invalid=invalid, device=gpu)
    src = torch.from_numpy(maps)
    src = with_pitch(src, g["raw"][1] + 5 if g["pitch"] is None else g["pitch"], gpu, 0xA5A5) if name != "upscale" else src.to(gpu)
    for augs in launches(g):
        buf, out = guarded((3, 1) + g["out"], gpu)
        lib.entry_log = log = []
        try:
            assert prep.prep_depth(src, augs, out=out) is out
        finally:
            lib.entry_log = None
        assert log == ["magnet_depth_prep_u16"]
        exp = torch.stack([ref.depth(maps[n], g["res"], g["out"], g["crop"], a.flip, a.window or (0, 0), divisor, invalid) for n, a in enumerate(augs)])
        got = out.cpu()
        mism = int((ref.bits(got) != ref.bits(exp)).sum())
        print(f"{name} / {divisor} / {invalid}: {mism} mismatches of {exp.numel()}")
        assert mism == 0 and guards_untouched(buf)
        if name != "tap_limit":                                   # 8 x 8 decimation keeps too few pixels to be sure of every value
            assert bool((exp == 0).any()) and (invalid is not None or bool((exp == float(np.float32(65535) / np.float32(divisor))).any()))


def test_c_abi_refusals(hip_lib, gpu):
    """Struct-level only: nothing launches, nothing is written."""
    src = torch.zeros(1, 97, 131, 3, dtype=torch.uint8, device=gpu)
    out = torch.zeros(1, 3, 40, 50, device=gpu)
    luts = ingest.normalise_table().to(gpu)[None].contiguous()
    rec = torch.zeros(1, 4, dtype=torch.int32, device=gpu)
    tab = torch.zeros(64 * 21, dtype=torch.int32, device=gpu)
    good = dict(src=src.data_ptr(), src_pitch=393, src_frame=393 * 97, luts=luts.data_ptr(), frame_params=rec.data_ptr(), out=out.data_ptr(),
                N=1, Hin=97, Win=131, crop_left=0, crop_top=0, crop_w=131, crop_h=97, Hres=48, Wres=64, Hout=40, Wout=50, kx=7, ky=7, n_luts=1,
                coef_x=tab.data_ptr(), bounds_x=tab.data_ptr(), coef_y=tab.data_ptr(), bounds_y=tab.data_ptr())
    call = lambda **kw: hip_lib.magnet_train_prep_u8(ctypes.byref(lib.MagnetTrainPrepArgs(**{**good, **kw})), None)
    assert hip_lib.magnet_train_prep_u8(None, None) == lib.E_NULL
    for k in ("src", "luts", "frame_params", "out"):
        assert call(**{k: None}) == lib.E_NULL, k
    for kw in (dict(N=0), dict(Hres=0), dict(Wres=32769), dict(Hout=49), dict(Wout=65), dict(Hout=0), dict(n_luts=0), dict(crop_left=1),
               dict(crop_h=98), dict(src_pitch=392), dict(kx=5), dict(ky=9)):
        assert call(**kw) == lib.E_DIM, kw
    assert call(Hres=10, Hout=10, ky=21) == lib.E_SHAPE and b"MAGNET_IMAGE_PREP_KMAX" in hip_lib.magnet_last_error()
    assert call(coef_y=None) == lib.E_NULL and call(bounds_x=None) == lib.E_NULL
    assert call(frame_params=rec.data_ptr() + 2) == lib.E_ALIGN and call(out=out.data_ptr() + 1) == lib.E_ALIGN
    assert call(Hres=97, Wres=131, coef_x=None, bounds_x=None, coef_y=None, bounds_y=None, Hout=0) == lib.E_DIM    # no tables needed, bad window

    dsrc = torch.zeros(1, 97, 131, dtype=torch.uint16, device=gpu)
    dout = torch.zeros(1, 1, 40, 50, device=gpu)
    dgood = dict(src=dsrc.data_ptr(), src_pitch=131, src_frame=131 * 97, idx_x=tab.data_ptr(), idx_y=tab.data_ptr(), frame_params=rec.data_ptr(),
                 out=dout.data_ptr(), N=1, Hin=97, Win=131, crop_left=0, crop_top=0, crop_w=131, crop_h=97, Hres=48, Wres=64, Hout=40, Wout=50,
                 invalid_code=-1, divisor=1000.0)
    dcall = lambda **kw: hip_lib.magnet_depth_prep_u16(ctypes.byref(lib.MagnetDepthPrepArgs(**{**dgood, **kw})), None)
    assert hip_lib.magnet_depth_prep_u16(None, None) == lib.E_NULL
    for k in ("src", "frame_params", "out"):
        assert dcall(**{k: None}) == lib.E_NULL, k
    for kw in (dict(N=65536), dict(Win=0), dict(Hout=49), dict(Wout=0), dict(crop_top=1), dict(src_pitch=130), dict(divisor=0.0),
               dict(divisor=-1.0), dict(divisor=float("inf")), dict(divisor=float("nan"))):
        assert dcall(**kw) == lib.E_DIM, kw
    assert dcall(idx_x=None) == lib.E_NULL and dcall(idx_y=None) == lib.E_NULL                     # a resized axis without its table
    assert dcall(Wres=131) == lib.E_NULL and dcall(Hres=97, Hout=40) == lib.E_NULL                # a table for an axis that is not resized
    assert dcall(idx_x=tab.data_ptr() + 2) == lib.E_ALIGN and dcall(src=dsrc.data_ptr() + 1) == lib.E_ALIGN
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(dout.any())


# ---- end to end against the loaders' host path ---------------------------------------------------------------------------------------
HW = (32, 48)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_prep_scene")
    _make_scene(str(root), "scene0007_00", 6, raw_wh=(131, 97))
    return str(root), [("scene0007_00", i) for i in (1, 2, 3, 4)]


def same_bits(dev_t, host_t):
    return dev_t.is_cuda and dev_t.dtype == host_t.dtype and dev_t.shape == host_t.shape and torch.equal(ref.bits(dev_t.cpu()), ref.bits(host_t))


def test_device_train_batches_equal_the_multi_view_host_path(hip_lib, gpu, scene):
    root, samples = scene
    kw = dict(n_views=2, window_radius=1, input_hw=HW, dpv_hw=(8, 12), augment=data.AugmentSpec(color=True), seed=2)
    host, raw = data.ScanNetFolder(root, samples, **kw), data.ScanNetFolder(root, samples, raw_images=True, **kw)
    prep = ingest.TrainPrep((97, 131), HW, device=gpu)
    coloured = 0
    for epoch in (0, 1):
        host.set_epoch(epoch); raw.set_epoch(epoch)
        before = (prep.uploads, prep.launches)
        loader = ingest.DeviceTrainBatches(list(data.batches(raw, 2)), prep)
        assert len(loader) == 2
        for (darr, dintr), (harr, hintr) in zip(loader, data.batches(host, 2)):
            assert len(darr) == len(harr) == 3
            for j, (d, h) in enumerate(zip(darr, harr)):
                assert set(d) == set(h) and same_bits(d["img"], h["img"]) and tuple(d["img"].shape) == (2, 3) + HW
                if j == 1:
                    assert same_bits(d["gt_dmap"], h["gt_dmap"]) and tuple(d["gt_dmap"].shape) == (2, 1) + HW
                else:
                    assert torch.equal(d["gt_dmap"], h["gt_dmap"])
                assert torch.equal(d["extM"], h["extM"]) and d["scene_name"] == h["scene_name"] and d["img_idx"] == h["img_idx"]
            assert all(torch.equal(dintr[k], hintr[k]) for k in hintr)
        # per batch: one upload shared by the frames' launch and the depth maps' launch
        assert (prep.uploads - before[0], prep.launches - before[1]) == (2, 4)
        coloured += sum(raw[i][0][0]["aug"].color is not None for i in range(len(samples)))
    assert 0 < coloured < 2 * len(samples) and prep.frames_prepared == 2 * 4 * 3 and prep.depths_prepared == 2 * 4


def test_device_train_batches_equal_the_single_view_host_path(hip_lib, gpu, scene):
    root, samples = scene
    spec = data.AugmentSpec(color=True, flip=True, crop_hw=(21, 34))
    host = data.ScanNetFrames(root, samples, input_hw=HW, augment=spec, seed=6)
    raw = data.ScanNetFrames(root, samples, input_hw=HW, augment=spec, seed=6, raw_images=True)
    preps = ingest.TrainPrepSet(HW, out_hw=spec.crop_hw, device=gpu)
    seen = set()
    for epoch in (0, 1, 2):
        host.set_epoch(epoch); raw.set_epoch(epoch)
        lib.entry_log = log = []
        try:
            got = list(ingest.DeviceTrainBatches(list(data.batches(raw, 2)), preps))
        finally:
            lib.entry_log = None
        assert log == ["magnet_train_prep_u8", "magnet_depth_prep_u16"] * 2
        for d, h in zip(got, data.batches(host, 2)):
            assert set(d) == set(h) == {"img", "depth", "scene_name", "img_idx"}
            assert same_bits(d["img"], h["img"]) and tuple(d["img"].shape) == (2, 3, 21, 34)
            assert same_bits(d["depth"], h["depth"]) and tuple(d["depth"].shape) == (2, 1, 21, 34)
            assert d["scene_name"] == h["scene_name"] and d["img_idx"] == h["img_idx"]
        seen |= {(a.flip, a.color is not None) for i in range(len(samples)) for a in [raw[i]["aug"]]}
    assert {f for f, _ in seen} == {False, True} and {c for _, c in seen} == {False, True}
    assert (preps.uploads, preps.launches, preps.frames_prepared, preps.depths_prepared) == (6, 12, 12, 12)
    # the 7-Scenes code and KITTI's divisor reach the kernel through the prep
    d16 = torch.tensor([[[65535, 1000], [256, 0]]], dtype=torch.uint16)
    seven = ingest.TrainPrep((2, 2), (2, 2), depth_invalid=65535, device=gpu).prep_depth(d16, [Augment(flip=True)])
    assert seven.cpu().flatten().tolist() == [1.0, 0.0, 0.0, float(np.float32(256) / np.float32(1000))]
    kitti = ingest.TrainPrep((2, 2), (2, 2), depth_divisor=256.0, device=gpu).prep_depth(d16, [Augment()])
    assert kitti.cpu().flatten().tolist() == [65535 / 256, 1000 / 256, 1.0, 0.0]
