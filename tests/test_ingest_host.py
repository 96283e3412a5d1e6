"""CPU: the host side of device image ingest (magnet_amd/ingest.py): the numpy restatement (tests/ingest_ref.py) against Pillow byte
for byte, the table builder and the lookup table against the restatement and the loader's expressions, the KITTI crop, every refusal,
and the loaders' raw_images mode.  No kernel runs here."""
import numpy as np
import pytest
import torch

from magnet_amd import data, ingest, lib
from magnet_amd.lib import MagnetError
from tests import ingest_ref
from tests.ingest_ref import OUT_HW, RAW_HW, make_image
from tests.test_data_loader import _make_scene


@pytest.mark.parametrize("kind", ["random", "binary", "ones"])
@pytest.mark.parametrize("raw_hw", RAW_HW)
def test_restatement_equals_pillow(raw_hw, kind):
    from PIL import Image
    img = make_image(kind, raw_hw, seed=raw_hw[0])
    exp = np.asarray(Image.fromarray(img).resize((OUT_HW[1], OUT_HW[0]), resample=Image.BILINEAR))
    got = ingest_ref.resize_u8(img, OUT_HW)
    assert got.dtype == np.uint8 and got.shape == exp.shape
    assert int((got != exp).sum()) == 0
    if raw_hw == OUT_HW:
        assert np.array_equal(got, img)


def test_restatement_tap_counts_and_clipped_windows():
    coef, bounds = ingest_ref.tables(131, 64)                     # ratio 2.05: ksize 2 * 3 + 1
    assert len(coef[0]) == 7 and bounds[0][0] == 0 and bounds[0][1] < 5 and sum(bounds[-1]) == 131 and bounds[-1][1] < 5
    assert max(n for _, n in bounds) in (5, 6) and all(sum(row) in range((1 << 22) - 4, (1 << 22) + 5) for row in coef)
    assert len(ingest_ref.tables(40, 64)[0][0]) == 3


def test_restatement_crop_equals_pillow():
    from PIL import Image
    img = make_image("random", (60, 150), seed=3)
    box = (11, 16, 128, 44)
    pil = Image.fromarray(img).crop((box[0], box[1], box[0] + box[2], box[1] + box[3]))
    assert np.array_equal(ingest_ref.resize_u8(img, (44, 128), crop=box), np.asarray(pil))
    exp = np.asarray(pil.resize((64, 30), resample=Image.BILINEAR))
    assert np.array_equal(ingest_ref.resize_u8(img, (30, 64), crop=box), exp)


@pytest.mark.parametrize("sizes", [(97, 48), (131, 64), (30, 48), (40, 64), (121, 48), (200, 64), (1296, 640), (968, 480), (512, 64), (199, 64)])
def test_resample_tables_equal_the_restatement(sizes):
    coef, bounds = ingest.resample_tables(*sizes)
    exp_coef, exp_bounds = ingest_ref.tables(*sizes)
    assert coef.dtype == np.int32 and bounds.dtype == np.int32 and coef.shape == (sizes[1], ingest.taps(*sizes))
    assert np.array_equal(coef, np.asarray(exp_coef, dtype=np.int32)) and np.array_equal(bounds, np.asarray(exp_bounds, dtype=np.int32))


def test_lookup_table_equals_the_loaders_expression():
    lut = ingest.normalise_table()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256)
    # data.ScanNetFolder.__getitem__'s lines on an image that holds every byte value, all 768 inputs
    v = np.arange(256, dtype=np.uint8)
    rgb = np.stack([v, v, v], axis=-1).reshape(16, 16, 3)
    mean = torch.tensor(data.IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(data.IMAGENET_STD).view(3, 1, 1)
    img = torch.from_numpy(np.asarray(rgb).astype(np.float32) / 255.0).permute(2, 0, 1)
    img = (img - mean) / std
    assert torch.equal(lut, img.reshape(3, 256))
    assert np.array_equal(lut.numpy(), ingest_ref.lookup(data.IMAGENET_MEAN, data.IMAGENET_STD))


def test_kitti_crop_matches_the_reference_margins():
    # dataloader_kitti.py:163-165: top = height - 352, left = int((width - 1216) / 2)
    for raw_hw, left, top in (((375, 1242), 13, 23), ((370, 1226), 5, 18)):
        p = ingest.ImagePrep.kitti(raw_hw)
        assert p.crop == (left, top, 1216, 352) and p.out_hw == (352, 1216)
        assert p._host["x"] is None and p._host["y"] is None      # a crop with no resize: both passes are skipped
    ci = data.cam_intrinsics_kitti(np.eye(3), 1242, 375, 88, 304)
    assert (float(ci["ray_params"][6]), float(ci["ray_params"][7])) == (13.0, 23.0)


def test_refusals():
    k = lib.IMAGE_PREP_KMAX
    assert k >= 9                                                # a downscale ratio of 4 must fit
    ingest.ImagePrep((8 * 48, 8 * 64), OUT_HW)                   # ratio 8: 17 taps, the limit
    with pytest.raises(MagnetError, match=f"IMAGE_PREP_KMAX = {k}") as e:
        ingest.ImagePrep((8 * 48 + 1, 64), OUT_HW)
    assert e.value.code == lib.E_SHAPE
    with pytest.raises(MagnetError, match="IMAGE_PREP_KMAX"):
        ingest.ImagePrep((48, 9 * 64), OUT_HW)
    for crop in ((-1, 0, 10, 10), (0, 0, 132, 10), (100, 0, 32, 10), (0, 90, 10, 8), (0, 0, 0, 10)):
        with pytest.raises(MagnetError, match="crop box"):
            ingest.ImagePrep((97, 131), OUT_HW, crop=crop)
    p = ingest.ImagePrep((97, 131), OUT_HW)
    with pytest.raises(MagnetError, match="uint8"):
        p.prep(torch.zeros(1, 97, 131, 3))
    with pytest.raises(MagnetError, match=r"\(N, Hin, Win, 3\)"):
        p.prep(torch.zeros(97, 131, 3, dtype=torch.uint8))
    with pytest.raises(MagnetError, match=r"\(N, Hin, Win, 3\)"):
        p.prep(torch.zeros(1, 3, 97, 131, dtype=torch.uint8))
    with pytest.raises(MagnetError, match="raw size"):
        p.prep(torch.zeros(1, 96, 131, 3, dtype=torch.uint8))
    frames = torch.zeros(2, 97, 131, 3, dtype=torch.uint8)
    with pytest.raises(MagnetError, match="out must be"):
        p.prep(frames, out=torch.zeros(2, 3, 48, 63))
    with pytest.raises(MagnetError, match="out must be"):
        p.prep(frames, out=torch.zeros(2, 3, 48, 64, dtype=torch.float64))
    with pytest.raises(MagnetError, match="out is on cpu"):
        p.prep(frames, out=torch.zeros(2, 3, 48, 64))
    assert p.frames_prepared == 0 and p.launches == 0


def test_runner_refuses_uint8_frames_without_a_prep():
    from magnet_amd.magnet import MAGNET
    from magnet_amd.sequence import SequenceRunner
    from magnet_amd.standin import StubDNet, StubFNet, make_args
    model = MAGNET(make_args(D=8, iters=1, dpv_h=8, dpv_w=8), d_net=StubDNet(1), f_net=StubFNet(2, fdim=16))
    with torch.no_grad():
        with pytest.raises(MagnetError, match="image_prep"):
            SequenceRunner(model, 4).add(["a"], torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
        with pytest.raises(MagnetError, match="image_prep must be"):
            SequenceRunner(model, 4, image_prep=object())
        r = SequenceRunner(model, 4, image_prep=ingest.ImagePrep((40, 48), (32, 32)))
        with pytest.raises(MagnetError, match="raw size"):
            r.add(["a"], torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
        assert r.prepared == 0 and r.pool is None


def test_raw_images_items_and_collate(tmp_path):
    from PIL import Image
    _make_scene(str(tmp_path), "scene0000_00", 8, raw_wh=(64, 48))
    _make_scene(str(tmp_path), "scene0001_00", 8, raw_wh=(80, 56))
    samples = [("scene0000_00", 3), ("scene0000_00", 4), ("scene0001_00", 3)]
    kw = dict(n_views=2, window_radius=2, input_hw=(32, 48), dpv_hw=(8, 12))
    ds, raw = data.ScanNetFolder(str(tmp_path), samples, **kw), data.ScanNetFolder(str(tmp_path), samples, raw_images=True, **kw)
    (arr, intr), (rarr, rintr) = ds[0], raw[0]
    for d, r in zip(arr, rarr):
        with Image.open(tmp_path / "scene0000_00" / "color" / (r["img_idx"] + ".jpg")) as im:
            decoded = np.asarray(im.convert("RGB"))
        assert r["img"].dtype == torch.uint8 and tuple(r["img"].shape) == (48, 64, 3) and np.array_equal(r["img"].numpy(), decoded)
        # the default item is today's: the host expressions on the Pillow resize of the same decoded frame
        exp = torch.from_numpy(np.asarray(Image.fromarray(decoded).resize((48, 32), resample=Image.BILINEAR)).astype(np.float32) / 255.0)
        exp = (exp.permute(2, 0, 1) - torch.tensor(data.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(data.IMAGENET_STD).view(3, 1, 1)
        assert d["img"].dtype == torch.float32 and torch.equal(d["img"], exp)
        # ... which is what the restatement makes of the raw item
        assert np.array_equal(ingest_ref.image_prep(r["img"].numpy()[None], (32, 48))[0], d["img"].numpy())
        assert set(d) == set(r) and d["img_idx"] == r["img_idx"] and d["scene_name"] == r["scene_name"] and np.array_equal(d["extM"], r["extM"])
        assert torch.equal(torch.as_tensor(d["gt_dmap"]), torch.as_tensor(r["gt_dmap"]))
    assert all(torch.equal(intr[k], rintr[k]) for k in intr)
    batch, _ = data.collate([raw[0], raw[1]])
    assert batch[0]["img"].dtype == torch.uint8 and tuple(batch[0]["img"].shape) == (2, 48, 64, 3)
    assert tuple(batch[1]["gt_dmap"].shape) == (2, 1, 32, 48)
    with pytest.raises(ValueError, match="raw frames of one batch"):
        data.collate([raw[0], raw[2]])
    seven = data.SevenScenesFolder(str(tmp_path), [], raw_images=True)
    assert seven.raw_images and not data.SevenScenesFolder(str(tmp_path), []).raw_images


def test_prepare_batch_refuses_mixed_raw_sizes():
    batch = ([{"img": torch.zeros(1, 48, 64, 3, dtype=torch.uint8)}, {"img": torch.zeros(1, 56, 80, 3, dtype=torch.uint8)}], {})
    with pytest.raises(MagnetError, match="one raw size"):
        ingest.prepare_batch(batch, ingest.ImagePrepSet((32, 48)))
