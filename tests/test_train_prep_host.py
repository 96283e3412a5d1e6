"""The host side of the training-sample preparation (magnet_amd/ingest.py: nearest_table, augment_table, TrainPrep's checks;
magnet_amd/data.py: AugmentSpec, draw_augment, the folders' training mode) against Pillow and numpy on whole images
(tests/train_prep_ref.py).  Every comparison is on all 32 bits: zero mismatches, no tolerance.  No GPU."""
import numpy as np
import pytest
import torch
from PIL import Image

from magnet_amd import data, ingest
from magnet_amd.lib import MagnetError
from tests import train_prep_ref as ref
from tests.test_data_loader import _make_scene

SIZES = [(1296, 640), (968, 480), (1000, 333), (700, 211), (41, 17), (17, 41), (97, 96), (64, 64), (1, 1)]


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_nearest_table_equals_pillow(n_in, n_out):
    """Pillow's NEAREST on I;16 ramps, along x and along y: the value of an output pixel is the index it was read from."""
    ramp = np.arange(n_in, dtype=np.uint16)
    table = ingest.nearest_table(n_in, n_out)
    assert table.dtype == np.int32 and table.shape == (n_out,)
    wide = Image.fromarray(np.tile(ramp[None], (3, 1)))
    tall = Image.fromarray(np.tile(ramp[:, None], (1, 3)))
    assert wide.mode == tall.mode == "I;16"
    assert np.array_equal(np.asarray(wide.resize((n_out, 3), resample=Image.NEAREST))[1], table)
    assert np.array_equal(np.asarray(tall.resize((3, n_out), resample=Image.NEAREST))[:, 1], table)
    with pytest.raises(MagnetError, match="positive"):
        ingest.nearest_table(n_in, 0)


def test_augment_table_equals_the_whole_image_expressions():
    """Looking the bytes of an image up in the table is the loaders' computation on that image, for the ends of the ranges, a
    product that clips, and 20 seeded draws; on a 480 x 640 image and on odd sizes."""
    images = [np.random.RandomState(3).randint(0, 256, hw + (3,), dtype=np.uint8) for hw in ((480, 640), (37, 53), (1, 257))]
    ramp = np.arange(256, dtype=np.uint8)
    images.append(np.stack([ramp, ramp[::-1], ramp], axis=-1)[None])          # every byte value in every channel
    draws = ref.COLOURS + ref.seeded_colours(20, seed=11)
    assert len(draws) >= 25
    clipped = 0
    for n, color in enumerate(draws):
        table = ingest.augment_table(color)
        assert table.dtype == torch.float32 and tuple(table.shape) == (3, 256)
        for img in images if n < 6 else images[1:]:                           # the large image with the range ends and one seeded draw
            exp = ref.normalise(ref.colour(img.astype(np.float32) / 255.0, *color))
            got = torch.stack([table[c][torch.from_numpy(img[..., c].astype(np.int64))] for c in range(3)])
            assert int((ref.bits(got) != ref.bits(exp)).sum()) == 0
        top = ref.normalise(np.ones((1, 1, 3), dtype=np.float32)).reshape(3)
        clipped += int(color[1] * max(color[2]) > 1.0 and bool((table[:, 255] == top).all()))
    assert clipped >= 2                                                       # the clip at 1 was exercised


def test_augment_table_without_a_draw_is_the_normalisation_table():
    assert torch.equal(ingest.augment_table(None), ingest.normalise_table())
    assert torch.equal(ingest.augment_table(), ingest.normalise_table())
    mean, std = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)
    assert torch.equal(ingest.augment_table(None, mean, std), ingest.normalise_table(mean, std))


def test_draw_augment_ranges_order_and_seeding():
    spec = data.AugmentSpec(color=True, flip=True, crop_hw=(416, 544))
    seen_flip, seen_color = set(), set()
    for i in range(200):
        a = data.draw_augment(spec, *data.augment_rngs(5, 2, i), (480, 640))
        assert isinstance(a, data.Augment) and isinstance(a.flip, bool)
        assert 0 <= a.window[0] <= 640 - 544 and 0 <= a.window[1] <= 480 - 416
        seen_flip.add(a.flip); seen_color.add(a.color is not None)
        if a.color is not None:
            g, b, cs = a.color
            assert 0.9 <= g <= 1.1 and 0.75 <= b <= 1.25 and len(cs) == 3 and all(0.9 <= c <= 1.1 for c in cs)
        assert a == data.draw_augment(spec, *data.augment_rngs(5, 2, i), (480, 640))           # the same (seed, epoch, index)
    assert seen_flip == {False, True} and seen_color == {False, True}
    draws = lambda s, e, i: data.draw_augment(spec, *data.augment_rngs(s, e, i), (480, 640))
    assert len({draws(5, 2, 7), draws(6, 2, 7), draws(5, 3, 7), draws(5, 2, 8)}) == 4
    # the documented order, replayed from generators in the same state: flip coin, crop x, crop y, colour coin, gamma, brightness,
    # then the three colours from numpy
    for i in range(40):
        py, nr = data.augment_rngs(9, 0, i)
        a = data.draw_augment(spec, *data.augment_rngs(9, 0, i), (480, 640))
        assert a.flip == (py.random() > 0.5)
        assert a.window == (py.randint(0, 640 - 544), py.randint(0, 480 - 416))
        if py.random() > 0.5:
            assert a.color[:2] == (py.uniform(0.9, 1.1), py.uniform(0.75, 1.25))
            assert a.color[2] == tuple(float(c) for c in nr.uniform(0.9, 1.1, size=3))
        else:
            assert a.color is None
    # KITTI's brightness range; a draw that is switched off consumes nothing
    for i in range(40):
        a = data.draw_augment(data.AugmentSpec(color=True, brightness=(0.9, 1.1)), *data.augment_rngs(1, 0, i), (352, 1216))
        assert a.flip is False and a.window is None and (a.color is None or 0.9 <= a.color[1] <= 1.1)
    py, nr = data.augment_rngs(1, 0, 0)
    state = py.getstate()
    assert data.draw_augment(data.AugmentSpec(), py, nr, (480, 640)) == data.Augment(None, False, None) and py.getstate() == state
    with pytest.raises(ValueError, match="does not fit"):
        data.draw_augment(data.AugmentSpec(crop_hw=(481, 640)), py, nr, (480, 640))


# ---- the folders ----------------------------------------------------------------------------------------------------------------
HW = (32, 48)
KW = dict(n_views=2, window_radius=1, input_hw=HW, dpv_hw=(8, 12))


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_scene")
    _make_scene(str(root), "scene0005_00", 6, raw_wh=(67, 51))
    return str(root), [("scene0005_00", i) for i in (1, 2, 3, 4)]


def _decoded(root, scene_name, k):
    sdir = f"{root}/{scene_name}"
    with Image.open(f"{sdir}/color/{k}.jpg") as im, Image.open(f"{sdir}/depth/{k}.png") as dm:
        return np.array(im.convert("RGB")), np.array(dm)


def _same_item(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def test_folder_without_augment_is_unchanged(scene):
    """augment=None: the items of both paths are what the plain constructor gives, and the all-off spec changes no host value."""
    root, samples = scene
    for raw in (False, True):
        plain = data.ScanNetFolder(root, samples, raw_images=raw, **KW)
        for other in (data.ScanNetFolder(root, samples, raw_images=raw, augment=None, seed=7, **KW),
                      data.ScanNetFolder(root, samples, augment=data.AugmentSpec(), **KW) if not raw else None):
            if other is None:
                continue
            for i in range(len(samples)):
                (arr, intr), (arr2, intr2) = plain[i], other[i]
                assert len(arr) == len(arr2) == 3
                for d, d2 in zip(arr, arr2):
                    _same_item(d, d2)
                _same_item(intr, intr2)
    arr, _ = data.ScanNetFolder(root, samples, **KW)[0]
    assert set(arr[1]) == {"img", "gt_dmap", "extM", "scene_name", "img_idx"}
    for j, d in enumerate(arr):                                               # and they are Pillow's and numpy's values
        frame, dmap = _decoded(root, d["scene_name"], int(d["img_idx"]))
        assert torch.equal(ref.bits(d["img"]), ref.bits(ref.image(frame, HW, HW)))
        assert torch.equal(ref.bits(d["gt_dmap"]), ref.bits(ref.depth(dmap, HW, HW))) if j == 1 else d["gt_dmap"] == 0.0


def test_multi_view_folder_host_path_equals_the_restatement(scene):
    root, samples = scene
    spec = data.AugmentSpec(color=True)
    ds = data.ScanNetFolder(root, samples, augment=spec, seed=3, **KW)
    raw = data.ScanNetFolder(root, samples, augment=spec, seed=3, raw_images=True, **KW)
    coloured = 0
    for epoch in (0, 1):
        ds.set_epoch(epoch); raw.set_epoch(epoch)
        for i in range(len(samples)):
            aug = data.draw_augment(spec, *data.augment_rngs(3, epoch, i), HW)
            coloured += aug.color is not None
            (arr, _), (rarr, _) = ds[i], raw[i]
            for j, (d, r) in enumerate(zip(arr, rarr)):
                frame, dmap = _decoded(root, d["scene_name"], int(d["img_idx"]))
                assert torch.equal(ref.bits(d["img"]), ref.bits(ref.image(frame, HW, HW, color=aug.color)))      # one draw for all views
                assert r["aug"] == aug and r["img"].dtype == torch.uint8 and np.array_equal(r["img"].numpy(), frame)
                if j == 1:
                    assert torch.equal(ref.bits(d["gt_dmap"]), ref.bits(ref.depth(dmap, HW, HW)))
                    assert "gt_dmap" not in r and r["gt_dmap_raw"].dtype == torch.uint16
                    assert np.array_equal(r["gt_dmap_raw"].numpy(), dmap)
                else:
                    assert d["gt_dmap"] == 0.0 and r["gt_dmap"] == 0.0 and "gt_dmap_raw" not in r
    assert 0 < coloured < 2 * len(samples)                                    # both branches of the colour coin were seen
    batch, _ = data.collate([raw[0], raw[1]])
    assert tuple(batch[1]["gt_dmap_raw"].shape) == (2, 51, 67) and batch[1]["gt_dmap_raw"].dtype == torch.uint16
    assert batch[0]["aug"] == [raw[0][0][0]["aug"], raw[1][0][0]["aug"]] and "gt_dmap_raw" not in batch[0]


def test_multi_view_folder_refuses_flip_and_crop(scene):
    root, samples = scene
    for spec in (data.AugmentSpec(flip=True), data.AugmentSpec(color=True, crop_hw=(16, 16))):
        with pytest.raises(ValueError, match="intrinsics"):
            data.ScanNetFolder(root, samples, augment=spec, **KW)
        with pytest.raises(ValueError, match="intrinsics"):
            data.SevenScenesFolder(root, samples, augment=spec, **KW)
    with pytest.raises(TypeError, match="AugmentSpec"):
        data.ScanNetFolder(root, samples, augment=True, **KW)


@pytest.mark.parametrize("spec", [None, data.AugmentSpec(color=True, flip=True, crop_hw=(21, 34)), data.AugmentSpec(flip=True),
                                  data.AugmentSpec(crop_hw=(32, 40))])
def test_single_view_frames_host_path_equals_the_restatement(scene, spec):
    root, samples = scene
    ds = data.ScanNetFrames(root, samples, input_hw=HW, augment=spec, seed=4)
    raw = data.ScanNetFrames(root, samples, input_hw=HW, augment=spec, seed=4, raw_images=True)
    out_hw = HW if spec is None or spec.crop_hw is None else spec.crop_hw
    seen = set()
    for epoch in (0, 1, 2):
        ds.set_epoch(epoch); raw.set_epoch(epoch)
        for i, (name, k) in enumerate(samples):
            aug = data.Augment() if spec is None else data.draw_augment(spec, *data.augment_rngs(4, epoch, i), HW)
            seen.add((aug.flip, aug.color is not None))
            frame, dmap = _decoded(root, name, k)
            item, ritem = ds[i], raw[i]
            assert set(item) == {"img", "depth", "scene_name", "img_idx"} and (item["scene_name"], item["img_idx"]) == (name, str(k))
            kw = dict(flip=aug.flip, window=aug.window or (0, 0))
            assert torch.equal(ref.bits(item["img"]), ref.bits(ref.image(frame, HW, out_hw, color=aug.color, **kw)))
            assert torch.equal(ref.bits(item["depth"]), ref.bits(ref.depth(dmap, HW, out_hw, **kw)))
            assert ritem["aug"] == aug and np.array_equal(ritem["img"].numpy(), frame) and np.array_equal(ritem["depth"].numpy(), dmap)
            assert ritem["depth"].dtype == torch.uint16
    if spec is not None and spec.flip:
        assert {f for f, _ in seen} == {False, True}
    batch = data.collate([raw[0], raw[1]])
    assert tuple(batch["img"].shape) == (2, 51, 67, 3) and tuple(batch["depth"].shape) == (2, 51, 67) and len(batch["aug"]) == 2
    with pytest.raises(ValueError, match="does not fit"):
        data.ScanNetFrames(root, samples, input_hw=HW, augment=data.AugmentSpec(crop_hw=(33, 48)))


def test_seven_scenes_frames_zero_the_invalid_code(tmp_path):
    sdir = tmp_path / "chess" / "seq-01"
    sdir.mkdir(parents=True)
    rng = np.random.RandomState(1)
    rgb = rng.randint(0, 256, (30, 40, 3), dtype=np.uint8)
    dmap = rng.randint(0, 3000, (30, 40)).astype(np.uint16)
    dmap[::3, ::2] = 65535
    Image.fromarray(rgb).save(sdir / "frame-000002.color.png")
    Image.fromarray(dmap).save(sdir / "frame-000002.depth.png")
    spec = data.AugmentSpec(flip=True, crop_hw=(20, 30))
    ds = data.SevenScenesFrames(str(tmp_path), [("chess", 1, 2)], input_hw=(24, 32), augment=spec, seed=1)
    assert (ds.depth_divisor, ds.depth_invalid, data.ScanNetFrames.depth_invalid) == (1000.0, 65535, None)
    for epoch in range(4):
        ds.set_epoch(epoch)
        aug = data.draw_augment(spec, *data.augment_rngs(1, epoch, 0), (24, 32))
        item = ds[0]
        exp = ref.depth(dmap, (24, 32), (20, 30), flip=aug.flip, window=aug.window, invalid=65535)
        assert torch.equal(ref.bits(item["depth"]), ref.bits(exp)) and bool((exp == 0).any()) and float(exp.max()) < 3.0
        assert torch.equal(ref.bits(item["img"]), ref.bits(ref.image(rgb, (24, 32), (20, 30), flip=aug.flip, window=aug.window)))


# ---- the Python layer's refusals: all raised on the host, before anything is uploaded -----------------------------------------------
def test_train_prep_refusals():
    A = data.Augment
    with pytest.raises(MagnetError, match=r"\(50, 40\).*\(48, 64\)"):
        ingest.TrainPrep((97, 131), (48, 64), out_hw=(50, 40))               # a crop larger than the resized image
    with pytest.raises(MagnetError, match="IMAGE_PREP_KMAX"):
        ingest.TrainPrep((48, 9 * 64), (48, 64))
    with pytest.raises(MagnetError, match="depth_divisor"):
        ingest.TrainPrep((97, 131), (48, 64), depth_divisor=0.0)
    p = ingest.TrainPrep((97, 131), (48, 64), out_hw=(40, 50))
    frames = torch.zeros(2, 97, 131, 3, dtype=torch.uint8)
    depth = torch.zeros(2, 60, 80, dtype=torch.uint16)
    for bad in (A(window=(15, 0)), A(window=(0, 9)), A(window=(-1, 0)), A(flip=True, window=(14, 8))):
        if bad.window == (14, 8):
            p.records([bad])                                                   # the largest origin is inside
            continue
        with pytest.raises(MagnetError, match=r"40 x 50 window at x=-?\d+ y=\d+ is not inside the resized 48 x 64"):
            p.prep(frames, [A(), bad])
        with pytest.raises(MagnetError, match="not inside the resized 48 x 64"):
            p.prep_depth(depth, [bad, A()])
    for augs in ([A()], [A(), A(), A()], []):
        with pytest.raises(MagnetError, match=rf"{len(augs)} Augments for 2 frames"):
            p.prep(frames, augs)
        with pytest.raises(MagnetError, match=rf"{len(augs)} Augments for 2 frames"):
            p.prep_depth(depth, augs)
    with pytest.raises(MagnetError, match="expected a magnet_amd.data.Augment"):
        p.prep(frames, [A(), (None, False, None)])
    with pytest.raises(MagnetError, match="uint8"):
        p.prep(frames.float(), [A(), A()])
    with pytest.raises(MagnetError, match=r"\(N, Hin, Win, 3\)"):
        p.prep(frames[0], [A()])
    with pytest.raises(MagnetError, match="raw size"):
        p.prep(frames[:, :90], [A(), A()])
    with pytest.raises(MagnetError, match="uint16"):
        p.prep_depth(depth.to(torch.int32), [A(), A()])
    with pytest.raises(MagnetError, match=r"\(N, Hd, Wd\)"):
        p.prep_depth(depth[0], [A()])
    k = ingest.TrainPrep.kitti((375, 1242))
    assert (k.resize_hw, k.out_hw, k.depth_divisor, k.images.crop) == ((352, 1216), (352, 1216), 256.0, (13, 23, 1216, 352))
    with pytest.raises(MagnetError, match="crop box made for frames"):
        k.depth_tables((370, 1242))
    luts, rec = p.records([A(), A(ref.COLOURS[0], True, (3, 4)), A(ref.COLOURS[1]), A(ref.COLOURS[0])])
    assert tuple(luts.shape) == (3, 3, 256) and torch.equal(luts[0], ingest.normalise_table())         # shared draws share a table
    assert rec.tolist() == [[0, 0, 0, 0], [1, 1, 3, 4], [2, 0, 0, 0], [1, 0, 0, 0]]
    assert (p.uploads, p.launches, p.frames_prepared) == (0, 0, 0)
    with pytest.raises(MagnetError, match="without 'aug'"):
        ingest.prepare_train_batch({"img": frames, "depth": depth}, p)
