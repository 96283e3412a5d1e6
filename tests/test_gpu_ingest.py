"""-m gpu: device image ingest (magnet_image_prep_u8, magnet_amd/ingest.py).  Every comparison is torch.equal: the kernel against
the numpy restatement of Pillow's arithmetic (tests/ingest_ref.py, itself held against Pillow in tests/test_ingest_host.py), ImagePrep
against the folder loader's host path, SequenceRunner and the driver's validate() with uint8 frames against host-normalised ones."""
import argparse

import numpy as np
import pytest
import torch

from magnet_amd import data, ingest, lib, synth
from magnet_amd.magnet import MAGNET
from magnet_amd.sequence import SequenceRunner
from magnet_amd.standin import StubDNet, StubFNet, make_args, seeded_magnet_weights
from tests import ingest_ref
from tests.ingest_ref import OUT_HW, RAW_HW, make_image
from tests.test_data_loader import _make_scene

pytestmark = pytest.mark.gpu


def frames_of(kinds, hw, seed):
    return np.stack([make_image(k, hw, seed + i) for i, k in enumerate(kinds)])


def check(gpu, frames, out_hw, crop=None, pitch=None):
    """prep(frames) on the device against the restatement; returns the device result."""
    N, H, W, _ = frames.shape
    prep = ingest.ImagePrep((H, W), out_hw, crop=crop, device=gpu)
    src = torch.from_numpy(frames).to(gpu)
    if pitch is not None:                                         # rows `pitch` bytes apart, the bytes between them poisoned
        wide = torch.full((N, H, pitch), 0xA5, dtype=torch.uint8, device=gpu)
        wide[:, :, :3 * W] = src.view(N, H, 3 * W)
        src = wide.as_strided((N, H, W, 3), (H * pitch, pitch, 3, 1))
        assert src.stride(1) == pitch and not src.is_contiguous()
    out = torch.full((N, 3) + tuple(out_hw), float("nan"), device=gpu)
    lib.entry_log = log = []
    try:
        assert prep.prep(src, out=out) is out
    finally:
        lib.entry_log = None
    assert log == ["magnet_image_prep_u8"]                        # one launch for all N frames
    exp = torch.from_numpy(ingest_ref.image_prep(frames, out_hw, crop))
    got = out.cpu()
    assert got.dtype == torch.float32 and got.shape == exp.shape
    assert int((got != exp).sum()) == 0 and torch.equal(got, exp)
    return out


@pytest.mark.parametrize("raw_hw", RAW_HW)
def test_kernel_equals_restatement(hip_lib, gpu, raw_hw):
    check(gpu, frames_of(("random", "binary", "random"), raw_hw, seed=10 + raw_hw[0]), OUT_HW)


def test_kernel_all_255_and_all_0(hip_lib, gpu):
    """The rounding term and the clamp: a constant image stays constant through both passes (coefficient rows that sum to 2^22 +- a
    few units of rounding), at the top and at the bottom of the range."""
    for raw_hw in ((97, 131), (30, 40)):
        out = check(gpu, frames_of(("ones", "zeros", "ones"), raw_hw, 0), OUT_HW)
        lut = ingest.normalise_table().to(gpu)
        for n, v in ((0, 255), (1, 0), (2, 255)):
            assert all(bool((out[n, c] == lut[c, v]).all()) for c in range(3))


def test_kernel_source_row_pitch(hip_lib, gpu):
    check(gpu, frames_of(("random", "random", "binary"), (97, 131), seed=5), OUT_HW, pitch=3 * 131 + 18)   # 411: every offset in a word


def test_kernel_crop_only(hip_lib, gpu):
    """The KITTI form: a crop with no resize, both passes skipped.  The pixels outside the box are never read: the result does not change
    when they do."""
    frames = frames_of(("random", "random", "random"), (60, 150), seed=7)
    box = (11, 16, 128, 44)
    out = check(gpu, frames, (44, 128), crop=box).clone()
    outside = frames.copy()
    keep = np.zeros((60, 150), dtype=bool); keep[16:60, 11:139] = True
    outside[:, ~keep] ^= 0xFF
    assert torch.equal(check(gpu, outside, (44, 128), crop=box), out)
    assert torch.equal(out[:, 0].cpu(), ingest.normalise_table()[0][torch.from_numpy(frames[:, 16:60, 11:139, 0].astype(np.int64))])


def test_kernel_crop_then_resize(hip_lib, gpu):
    check(gpu, frames_of(("random", "binary", "random"), (60, 150), seed=8), (30, 64), crop=(11, 16, 128, 44))
    check(gpu, frames_of(("random", "random", "random"), (60, 150), seed=9), (44, 64), crop=(11, 16, 128, 44))   # horizontal pass only


def test_kernel_many_tiles_and_the_tap_limit(hip_lib, gpu):
    """More than two tiles along both axes with sizes no tile divides; a downscale ratio of 8, the kernel's limit of taps, where the
    staged rows of a tile are the most the LDS stage holds."""
    check(gpu, frames_of(("random", "binary"), (75, 400), seed=11), (33, 170))
    check(gpu, frames_of(("random", "ones"), (8 * 48, 8 * 64), seed=12), OUT_HW)
    assert ingest.taps(8 * 48, 48) == lib.IMAGE_PREP_KMAX


def test_c_abi_refusals(hip_lib, gpu):
    import ctypes
    src = torch.zeros(1, 97, 131, 3, dtype=torch.uint8, device=gpu)
    out = torch.zeros(1, 3, 10, 64, device=gpu)
    lut = ingest.normalise_table().to(gpu)
    tab = torch.zeros(64 * 21, dtype=torch.int32, device=gpu)
    a = lib.MagnetImagePrepArgs(src=src.data_ptr(), src_pitch=393, src_frame=393 * 97, lut=lut.data_ptr(), out=out.data_ptr(), N=1, Hin=97,
                                Win=131, crop_left=0, crop_top=0, crop_w=131, crop_h=97, Hout=10, Wout=64, kx=7, ky=21,
                                coef_x=tab.data_ptr(), bounds_x=tab.data_ptr(), coef_y=tab.data_ptr(), bounds_y=tab.data_ptr())
    assert hip_lib.magnet_image_prep_u8(ctypes.byref(a), None) == lib.E_SHAPE        # 97 -> 10 rows: 21 taps
    assert b"MAGNET_IMAGE_PREP_KMAX" in hip_lib.magnet_last_error()
    a.Hout, a.ky, a.crop_left = 48, 7, 1
    assert hip_lib.magnet_image_prep_u8(ctypes.byref(a), None) == lib.E_DIM          # the box leaves the frame
    a.crop_left, a.src_pitch = 0, 392
    assert hip_lib.magnet_image_prep_u8(ctypes.byref(a), None) == lib.E_DIM
    a.src_pitch, a.kx = 393, 5
    assert hip_lib.magnet_image_prep_u8(ctypes.byref(a), None) == lib.E_DIM          # not the row length the sizes imply
    a.kx, a.coef_y = 7, None
    assert hip_lib.magnet_image_prep_u8(ctypes.byref(a), None) == lib.E_NULL
    torch.cuda.synchronize()
    assert not bool(out.any())                                                       # a refused call writes nothing


# ---- end to end against the loader -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Six frames of 131 x 97, four windows of V = 2 that share frames; the default folder and its raw_images twin."""
    root = tmp_path_factory.mktemp("ingest_scene")
    _make_scene(str(root), "scene0003_00", 6, raw_wh=(131, 97))
    samples = [("scene0003_00", i) for i in (1, 2, 3, 4)]
    kw = dict(n_views=2, window_radius=1, input_hw=OUT_HW, dpv_hw=(OUT_HW[0] // 4, OUT_HW[1] // 4))
    return data.ScanNetFolder(str(root), samples, **kw), data.ScanNetFolder(str(root), samples, raw_images=True, **kw)


def test_image_prep_equals_the_loader(hip_lib, gpu, folder):
    ds, raw = folder
    prep = ingest.ImagePrep((97, 131), OUT_HW, device=gpu)
    pinned_seen = False
    for i in range(len(ds)):
        (arr, _), (rarr, _) = ds[i], raw[i]
        exp = torch.stack([d["img"] for d in arr])
        frames = torch.stack([d["img"] for d in rarr])
        assert frames.dtype == torch.uint8 and not frames.is_cuda
        from_cpu = prep.prep(frames.pin_memory() if i % 2 else frames)
        pinned_seen |= bool(i % 2)
        from_gpu = prep.prep(frames.to(gpu))
        assert from_cpu.is_cuda and torch.equal(from_cpu, from_gpu)
        assert int((from_gpu.cpu() != exp).sum()) == 0 and torch.equal(from_gpu.cpu(), exp)
    assert pinned_seen and prep.frames_prepared == 2 * 3 * len(ds) and prep.launches == 2 * len(ds)


# ---- SequenceRunner ------------------------------------------------------------------------------------------------------------------
def stub_model(gpu):
    args = make_args(D=8, iters=2, dpv_h=OUT_HW[0] // 4, dpv_w=OUT_HW[1] // 4, V=2)
    args.min_depth, args.max_depth = 1e-3, 10.0
    model = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2)).to(gpu).eval()
    seeded_magnet_weights(model, 3)
    return model, args


def window(ref, gpu):
    refs, nghbrs = [ref], [ref - 1, ref + 1]
    poses = synth.make_poses("scannet", 1, 2, torch.Generator().manual_seed(700 + ref)).to(gpu)
    return refs, nghbrs, poses, torch.ones(1, 2, dtype=torch.int32), synth.make_intrinsics("scannet", OUT_HW[0] // 4, OUT_HW[1] // 4, 1)


@pytest.mark.parametrize("graph", [False, True])
def test_sequence_runner_takes_uint8_frames(hip_lib, gpu, graph):
    raw = torch.from_numpy(frames_of(("random",) * 5, (97, 131), seed=40))
    host = torch.from_numpy(ingest_ref.image_prep(raw.numpy(), OUT_HW)).to(gpu)      # what the loader's host path hands over
    (m_ref, _), (m_dev, _) = stub_model(gpu), stub_model(gpu)
    prep = ingest.ImagePrep((97, 131), OUT_HW, device=gpu)
    plain, fed = SequenceRunner(m_ref, 8, graph=graph), SequenceRunner(m_dev, 8, graph=graph, image_prep=prep)
    raw_gpu = raw.to(gpu)
    launches = []
    with torch.no_grad():
        for ref in (1, 2, 3):                                    # overlapping windows: 3 new frames, then 1, then 1
            refs, nghbrs, *rest = window(ref, gpu)
            exp = [p.clone() for p in plain.forward(refs, host[refs], nghbrs, host[nghbrs], *rest)]
            # the first two calls hand over host tensors: three new frames in two runs (uploaded run by run), then one
            src = raw if ref in (1, 2) else raw_gpu
            lib.entry_log = log = []
            try:
                got = [p.clone() for p in fed.forward(refs, src[refs], nghbrs, src[nghbrs], *rest)]
            finally:
                lib.entry_log = None
            launches.append(log.count("magnet_image_prep_u8"))
            assert len(got) == len(exp) == 2 and all(torch.equal(g, e) for g, e in zip(got, exp)), ref
            assert bool(torch.isfinite(got[-1]).all())
            assert (fed.prepared, prep.frames_prepared) == ({1: 3, 2: 4, 3: 5}[ref],) * 2
    assert launches == [1, 1, 1] and fed.encoded == plain.encoded == 5
    with torch.no_grad():                                        # nothing new: nothing prepared, nothing launched for it
        refs, nghbrs, *rest = window(2, gpu)
        again = fed.forward(refs, raw_gpu[refs], nghbrs, raw_gpu[nghbrs], *rest)
        assert all(torch.equal(g, e) for g, e in zip(again, plain.forward(refs, host[refs], nghbrs, host[nghbrs], *rest)))
    assert fed.prepared == 5 and prep.launches == 3
    assert torch.equal(fed.pool.feat, plain.pool.feat) and torch.equal(fed.pool.gmm, plain.pool.gmm) and bool(fed.pool.feat.any())
    if graph:
        assert fed.graph_stats == plain.graph_stats and sum(fed.graph_stats["replays"].values()) > 0


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_validate_with_device_images_gives_the_same_metrics(hip_lib, gpu, folder):
    import eval_synthetic
    ds, raw = folder
    model, args = stub_model(gpu)
    a = argparse.Namespace(input_height=OUT_HW[0], input_width=OUT_HW[1])
    ref = eval_synthetic.validate(model, args, eval_synthetic.FolderBatches(ds, 2), gpu)
    loader, preps = ingest.device_image_loader(a, eval_synthetic.FolderBatches(raw, 2), gpu)
    got = eval_synthetic.validate(model, args, loader, gpu)
    assert set(ref) == set(got) and len(ref) >= 9 and all(np.isfinite(v) for v in ref.values())
    assert {k: float(v).hex() for k, v in got.items()} == {k: float(v).hex() for k, v in ref.items()}
    assert preps.frames_prepared == 4 * 3 and preps.launches == 2                    # one launch per batch of 2 windows x 3 frames
    # through a frame pool: the runner prepares each of the 6 frames once
    plain = eval_synthetic.validate(model, args, eval_synthetic.FolderBatches(ds, 2), gpu, runner=SequenceRunner(model, 6))
    loader, preps = ingest.device_image_loader(a, eval_synthetic.FolderBatches(raw, 2), gpu, to_runner=True)
    runner = SequenceRunner(model, 6, image_prep=preps)
    pooled = eval_synthetic.validate(model, args, loader, gpu, runner=runner)
    assert {k: float(v).hex() for k, v in pooled.items()} == {k: float(v).hex() for k, v in plain.items()}
    assert runner.prepared == runner.encoded == 6
