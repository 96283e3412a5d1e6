#!/usr/bin/env python3
"""test_DNet.py-shaped driver for the stand-alone D-Net (the counterpart of eval_synthetic.py for the reference's test_DNet.py:22-73).

Same flow as the reference's validate(): loader -> model(img) -> split (mu, variance) -> clamp + mask -> depth metrics with the NLL
term -> running average -> log_metrics line.  Differences: frames come from a seeded synthetic generator of single images or from
magnet_amd/data.py's folders (the reference frame of each window), the encoder is caller-provided (the stand-in here), the decoder,
heads and tail run on the HIP path (DNET(dnet=True, backend='hip')), and the metric reductions run on the device.

    python eval_dnet.py --frames 8 [--batch 1] [--backend hip] [--log out.txt]
    python eval_dnet.py --dataset_path ROOT --split split.txt [--dataset_format 7scenes] [--device_images]
    python eval_dnet.py --sharded [--gpus N] [--dist_backend gloo] [--dump_metrics out.json]     (or under torch.distributed.run)
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from magnet_amd import evaluate as E  # noqa: E402
from magnet_amd import ingest  # noqa: E402
from magnet_amd import metrics as M  # noqa: E402


class SyntheticFrames:
    """Yields dicts like the reference's single-view loaders (data/dataloader_scannet_D.py): 'img' (B,3,H,W), 'depth' (B,1,H,W);
    seeded, depth in [1, 4) m with a band of missing measurements (zeros) at the top of every frame."""

    def __init__(self, n_frames, batch, H, W, seed=0):
        self.n, self.B, self.H, self.W, self.seed = n_frames, batch, H, W, seed

    def __len__(self):
        return (self.n + self.B - 1) // self.B

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for s in range(0, self.n, self.B):
            b = min(self.B, self.n - s)
            depth = torch.rand(b, 1, self.H, self.W, generator=g) * 3 + 1
            depth[:, :, :self.H // 16] = 0.0
            yield {"img": torch.rand(b, 3, self.H, self.W, generator=g), "depth": depth}


class FolderFrames:
    """The reference frame of every window of a magnet_amd.data folder dataset, as single-view batches."""

    def __init__(self, dataset, batch):
        self.ds, self.B = dataset, batch

    def __len__(self):
        return (len(self.ds) + self.B - 1) // self.B

    def __iter__(self):
        for s in range(0, len(self.ds), self.B):
            refs = [self.ds[i][0][self.ds.center] for i in range(s, min(s + self.B, len(self.ds)))]
            yield {"img": torch.stack([r["img"] for r in refs]), "depth": torch.stack([r["gt_dmap"] for r in refs])}


def validate(model, args, test_loader, device):
    """The reference's validate() (test_DNet.py:22-73), metrics reduced on the device.  The metric kernel takes (mu, sigma), squares
    sigma and clamps the variance at 1e-6 as utils.py:133 does; every frame of a batch is evaluated (the reference runs batch 1)."""
    with torch.no_grad():
        metrics = M.RunningAverageDict()
        crop = "garg" if getattr(args, "garg_crop", False) else ("eigen" if getattr(args, "eigen_crop", False) else None)
        for t_data_dict in test_loader:
            img = t_data_dict["img"].to(device)
            gt_dmap = t_data_dict["depth"].to(device)
            out = model(img)                                                        # (B, 2, H, W) [mu, variance]
            pred_dmap, pred_var = torch.split(out, 1, dim=1)
            pred = torch.cat([pred_dmap, torch.sqrt(pred_var)], dim=1)
            for m in M.compute_depth_errors(pred, gt_dmap, args.min_depth, args.max_depth, crop=crop):   # test_DNet.py:51-71
                metrics.update(m)
        return metrics.get_value()


def validate_sharded(model, args, test_loader, device, rank=0, world=1, with_count=False):
    """validate() over this rank's share of the batches with the metric rows kept on the device: the model's (mu, variance) goes to the
    metric kernel as it is (kind='variance': the clamp of utils.py:133 applies to the variance itself, no sqrt / square round trip),
    nothing is read back per batch, and the rows of all ranks are gathered once and averaged in loader order."""
    with torch.no_grad():
        crop = "garg" if getattr(args, "garg_crop", False) else ("eigen" if getattr(args, "eigen_crop", False) else None)
        table = M.MetricTable(device, args.min_depth, args.max_depth, crop=crop, kind="variance")

        def step(t_data_dict):
            img = t_data_dict["img"].to(device)
            gt_dmap = t_data_dict["depth"].to(device)
            table.append_pred(model(img), gt_dmap)                                  # (B, 2, H, W) [mu, variance]

        metrics, n = E.evaluate(step, test_loader, table, rank, world)
        return (metrics, n) if with_count else metrics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8); ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--input_height", type=int, default=480); ap.add_argument("--input_width", type=int, default=640)
    ap.add_argument("--min_depth", type=float, default=1e-3); ap.add_argument("--max_depth", type=float, default=10.0)
    ap.add_argument("--backend", default="hip", choices=["hip", "torch"]); ap.add_argument("--log", default="")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--split_k", default="0", choices=["0", "auto"],
                    help="split-K launches for the decoder's plain layers (DNetMFMA(split_k=...)); needs --backend hip")
    ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "fp16"],
                    help="operand format of the HIP decoder (DNetMFMA(precision=...)): fp16 = one fp16 plane per buffer, reduced precision, "
                         "|activation| <= 65504 or clamped; needs --backend hip")
    ap.add_argument("--dataset_path", default="", help="root of ScanNet-format scene folders (magnet_amd/data.py) instead of synthetic frames")
    ap.add_argument("--split", default="", help="text file of '<scene> <frame index>' lines (data_split/scannet_*.txt format)")
    ap.add_argument("--dataset_format", default="scannet", choices=["scannet", "7scenes"],
                    help="folder layout; the split file has '<scene> <frame>' or '<scene> <sequence> <frame>' lines")
    ap.add_argument("--garg_crop", action="store_true", help="KITTI: evaluate inside the Garg ECCV16 window (test_DNet.py:56-58)")
    ap.add_argument("--eigen_crop", action="store_true", help="KITTI: evaluate inside the Eigen NIPS14 window (test_DNet.py:59-61)")
    ap.add_argument("--encoder", default="standin", choices=["standin", "b5"],
                    help="'standin' (default): the seeded stand-in encoder; 'b5': the EfficientNet-B5 encoder (magnet_amd/encoder.py), calibrated seeded weights")
    ap.add_argument("--encoder_backend", default="torch", choices=["torch", "hip"], help="with --encoder b5: run the encoder's torch modules or EncoderMFMA")
    ap.add_argument("--encoder_precision", default="bf16x3", choices=["bf16x3", "fp16"],
                    help="with --encoder b5 --encoder_backend hip: EncoderMFMA's format; fp16 = one fp16 plane per activation grid, reduced "
                         "precision, |activation| <= 65504 or clamped")
    E.add_arguments(ap)
    ingest.add_arguments(ap)
    a = ap.parse_args()
    if a.device_images and not a.dataset_path:
        ap.error("--device_images needs --dataset_path: the synthetic frames are normalised images already")
    if a.encoder_backend == "hip" and a.encoder != "b5":
        ap.error("--encoder_backend hip is a mode of --encoder b5")
    if a.encoder_precision != "bf16x3" and not (a.encoder == "b5" and a.encoder_backend == "hip"):
        ap.error("--encoder_precision fp16 is a mode of --encoder b5 --encoder_backend hip")
    rank, world, device, sharded = E.start(a, __file__)
    from magnet_amd.standin import make_dnet
    args = argparse.Namespace(min_depth=a.min_depth, max_depth=a.max_depth, garg_crop=a.garg_crop, eigen_crop=a.eigen_crop)
    model = make_dnet(dnet=True, backend=a.backend, split_k="auto" if a.split_k == "auto" else 0, precision=a.precision,
                      encoder=a.encoder, encoder_backend=a.encoder_backend, encoder_precision=a.encoder_precision).to(device).eval()    # seeded weights unless the caller loads a checkpoint
    if a.dataset_path:
        from magnet_amd import data
        with open(a.split) as f:
            samples = [ln.split()[:3 if a.dataset_format == "7scenes" else 2] for ln in f if ln.strip()]
        Folder = data.SevenScenesFolder if a.dataset_format == "7scenes" else data.ScanNetFolder
        # window_radius 0: every window entry is the reference frame itself, so no neighbour has to exist
        ds = Folder(a.dataset_path, samples, n_views=2, window_radius=0, input_hw=(a.input_height, a.input_width),
                    dpv_hw=(a.input_height // 4, a.input_width // 4), **({"raw_images": True} if a.device_images else {}))
        loader = FolderFrames(ds, a.batch)
        if a.device_images:
            loader, _ = ingest.device_image_loader(a, loader, device)
        title = "%s-format folder %s (%d frames) D-Net backend=%s" % (a.dataset_format, a.dataset_path, len(ds), a.backend)
    else:
        loader = SyntheticFrames(a.frames, a.batch, a.input_height, a.input_width, seed=a.seed)
        title = "synthetic frames=%d D-Net backend=%s" % (a.frames, a.backend)
    if not sharded:
        M.log_metrics(a.log, validate(model, args, loader, device), title)
        return
    m, n = validate_sharded(model, args, loader, device, rank, world, with_count=True)
    if rank == 0:
        M.log_metrics(a.log, m, title)
        if a.dump_metrics:
            E.dump_metrics(a.dump_metrics, m, n)
    E.finish()


if __name__ == "__main__":
    main()
