#!/usr/bin/env python3
"""The validate() of the reference's F-Net driver (train_FNet.py:148-195) as a driver of its own (the counterpart of eval_dnet.py).

Same flow: loader -> data_preprocess -> MAGNET_F(ref_img, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, d_center) in .eval() ->
expected depth under the softmax over the bins -> nearest upsampling to the image size -> clamp + mask (+ KITTI crops) -> depth
metrics -> running average -> log_metrics line.  Differences: windows come from a seeded synthetic generator or from
magnet_amd/data.py's folders, the F-Net runs on the matrix cores (train_backend='hip' in .eval()), the model returns the raw volume
and homography.expected_depth_F fuses softmax and expectation in one pass, and the metric reductions run on the device.  The metric
kernel takes (mu, sigma): sigma = 1 is passed and nll is reported as 0.0, as utils.compute_depth_errors(..., None) does.

    python eval_fnet.py --frames 8 [--batch 1] [--V 4] [--D 80] [--log out.txt]
    python eval_fnet.py --dataset_path ROOT --split split.txt [--dataset_format 7scenes] [--device_images]
    python eval_fnet.py --sharded [--gpus N] [--dist_backend gloo] [--dump_metrics out.json]     (or under torch.distributed.run)
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from magnet_amd import evaluate as E  # noqa: E402
from magnet_amd import ingest  # noqa: E402
from magnet_amd import metrics as M  # noqa: E402
from magnet_amd.homography import expected_depth_F  # noqa: E402
from magnet_amd.preprocess import data_preprocess_device  # noqa: E402


def sid_centres(n_depths, min_depth, max_depth):
    """The driver's bin centres (train_FNet.py:56-66): spacing-increasing discretisation, (1, n_depths, 1, 1) fp32."""
    d_gamma = 1 - min_depth
    d_boundaries = np.exp(np.log(max_depth + d_gamma) * np.arange(n_depths + 1) / n_depths) - d_gamma
    d_center = (d_boundaries[:-1] + d_boundaries[1:]) / 2
    return torch.from_numpy(d_center.astype(np.float32)).view(1, n_depths, 1, 1)


def validate(model, args, test_loader, device, d_center):
    """The reference's validate() (train_FNet.py:148-195), metrics reduced on the device; every frame of a batch is evaluated (the
    reference reads frame 0 of a batch of 1)."""
    with torch.no_grad():
        metrics = M.RunningAverageDict()
        crop = "garg" if getattr(args, "garg_crop", False) else ("eigen" if getattr(args, "eigen_crop", False) else None)
        for data_array, cam_intrins in test_loader:
            cur_batch_size = data_array[0]["img"].size()[0]
            ref_dat, nghbr_dats, nghbr_poses, is_valid = data_preprocess_device(data_array, cur_batch_size, device)
            ref_img = ref_dat["img"].to(device)
            gt_dmap = ref_dat["gt_dmap"].to(device)
            gt_dmap[gt_dmap > args.max_depth] = 0.0
            nghbr_imgs = torch.cat([d["img"].to(device) for d in nghbr_dats], dim=0)       # view-major
            raw = model(ref_img, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, d_center, softmax=False)
            pred_dmap = expected_depth_F(raw, d_center)                                  # train_FNet.py:166-167
            pred_dmap = F.interpolate(pred_dmap, size=[ref_img.shape[2], ref_img.shape[3]], mode="nearest")
            pred = torch.cat([pred_dmap, torch.ones_like(pred_dmap)], dim=1)             # (mu, sigma = 1)
            for m in M.compute_depth_errors(pred, gt_dmap, args.min_depth, args.max_depth, crop=crop):   # train_FNet.py:175-193
                m["nll"] = 0.0
                metrics.update(m)
        return metrics.get_value()


def validate_sharded(model, args, test_loader, device, d_center, rank=0, world=1, with_count=False):
    """validate() over this rank's share of the batches with the metric rows kept on the device: the expected-depth map goes to the
    metric kernel alone (kind=None: no plane of ones, nll 0.0 written by the kernel), nothing is read back per batch, and the rows of
    all ranks are gathered once and averaged in loader order."""
    with torch.no_grad():
        crop = "garg" if getattr(args, "garg_crop", False) else ("eigen" if getattr(args, "eigen_crop", False) else None)
        table = M.MetricTable(device, args.min_depth, args.max_depth, crop=crop, kind=None)

        def step(batch):
            data_array, cam_intrins = batch
            cur_batch_size = data_array[0]["img"].size()[0]
            ref_dat, nghbr_dats, nghbr_poses, is_valid = data_preprocess_device(data_array, cur_batch_size, device)
            ref_img = ref_dat["img"].to(device)
            gt_dmap = ref_dat["gt_dmap"].to(device)                                      # gt > max_depth is masked by the kernel
            nghbr_imgs = torch.cat([d["img"].to(device) for d in nghbr_dats], dim=0)       # view-major
            raw = model(ref_img, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, d_center, softmax=False)
            pred_dmap = expected_depth_F(raw, d_center)
            pred_dmap = F.interpolate(pred_dmap, size=[ref_img.shape[2], ref_img.shape[3]], mode="nearest")
            table.append(pred_dmap, gt_dmap)

        metrics, n = E.evaluate(step, test_loader, table, rank, world)
        return (metrics, n) if with_count else metrics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8); ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--V", type=int, default=4); ap.add_argument("--D", type=int, default=80)
    ap.add_argument("--input_height", type=int, default=480); ap.add_argument("--input_width", type=int, default=640)
    ap.add_argument("--min_depth", type=float, default=1e-3); ap.add_argument("--max_depth", type=float, default=10.0)
    ap.add_argument("--log", default=""); ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dataset_path", default="", help="root of ScanNet-format scene folders (magnet_amd/data.py) instead of synthetic frames")
    ap.add_argument("--split", default="", help="text file of '<scene> <frame index>' lines (data_split/scannet_*.txt format)")
    ap.add_argument("--window_radius", type=int, default=20)
    ap.add_argument("--dataset_format", default="scannet", choices=["scannet", "7scenes"],
                    help="folder layout; the split file has '<scene> <frame>' or '<scene> <sequence> <frame>' lines")
    ap.add_argument("--garg_crop", action="store_true", help="KITTI: evaluate inside the Garg ECCV16 window (train_FNet.py:180-181)")
    ap.add_argument("--eigen_crop", action="store_true", help="KITTI: evaluate inside the Eigen NIPS14 window (train_FNet.py:182-183)")
    E.add_arguments(ap)
    ingest.add_arguments(ap)
    a = ap.parse_args()
    if a.device_images and not a.dataset_path:
        ap.error("--device_images needs --dataset_path: the synthetic frames are normalised images already")
    rank, world, device, sharded = E.start(a, __file__)
    from magnet_amd.magnet import MAGNET_F
    args = argparse.Namespace(min_depth=a.min_depth, max_depth=a.max_depth, garg_crop=a.garg_crop, eigen_crop=a.eigen_crop,
                              FNET_architecture="PSM-Net", FNET_feature_dim=64)
    torch.manual_seed(a.seed)
    model = MAGNET_F(args, train_backend="hip").to(device).eval()         # seeded weights unless the caller loads a checkpoint
    d_center = sid_centres(a.D, a.min_depth, a.max_depth).to(device)
    if a.dataset_path:
        from magnet_amd import data
        with open(a.split) as f:
            samples = [ln.split()[:3 if a.dataset_format == "7scenes" else 2] for ln in f if ln.strip()]
        Folder = data.SevenScenesFolder if a.dataset_format == "7scenes" else data.ScanNetFolder
        ds = Folder(a.dataset_path, samples, n_views=a.V, window_radius=a.window_radius, input_hw=(a.input_height, a.input_width),
                    dpv_hw=(a.input_height // 4, a.input_width // 4), **({"raw_images": True} if a.device_images else {}))
        loader = data.batches(ds, a.batch)
        if a.device_images:
            loader, _ = ingest.device_image_loader(a, loader, device)
        title = "%s-format folder %s (%d windows) F-Net V=%d D=%d" % (a.dataset_format, a.dataset_path, len(ds), a.V, a.D)
    else:
        from eval_synthetic import SyntheticWindows
        loader = SyntheticWindows((a.frames + a.batch - 1) // a.batch, a.batch, a.V, a.input_height, a.input_width, seed=a.seed)
        title = "synthetic frames=%d F-Net V=%d D=%d" % (a.frames, a.V, a.D)
    if not sharded:
        M.log_metrics(a.log, validate(model, args, loader, device, d_center), title)
        return
    m, n = validate_sharded(model, args, loader, device, d_center, rank, world, with_count=True)
    if rank == 0:
        M.log_metrics(a.log, m, title)
        if a.dump_metrics:
            E.dump_metrics(a.dump_metrics, m, n)
    E.finish()


if __name__ == "__main__":
    main()
