#!/usr/bin/env python3
"""test_MaGNet.py-shaped driver on synthetic frames (SURVEY.md §8b "Python-side counterpart"; BASELINE config 1).

Same flow as the reference's validate() (test_MaGNet.py:27-81): loader -> data_preprocess -> model(ref_img,
nghbr_imgs, nghbr_poses, is_valid, cam_intrins, mode='test') -> clamp + mask -> depth metrics -> running average ->
log_metrics line.  Differences: frames come from a seeded synthetic window generator instead of the dataset loaders,
the backbones are caller-provided (stub D-Net/F-Net here), and the metric reductions run on the device.

    python eval_synthetic.py --frames 8 --batch 2 [--D 5] [--iters 3] [--V 4] [--log out.txt]
    python eval_synthetic.py --sharded [--gpus N] [--dist_backend gloo] [--dump_metrics out.json]     (or under torch.distributed.run)
    python eval_synthetic.py --dataset_path ROOT --split split.txt --reuse_backbones [--pool_frames 64] [--graph]
    python eval_synthetic.py --dataset_path ROOT --split split.txt --device_images [--reuse_backbones]
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
from magnet_amd import synth  # noqa: E402
from magnet_amd.magnet import MAGNET  # noqa: E402
from magnet_amd.preprocess import data_preprocess, data_preprocess_device, split_data_array  # noqa: E402,F401


class SyntheticWindows:
    """Yields (data_array, cam_intrins) like ScannetLoader(...).data (data/dataloader_scannet.py:155-217): a list of
    V+1 dicts with 'img' (B,3,H,W), 'gt_dmap' (B,1,H,W), 'extM' (B,4,4 float64), reference frame in the middle."""

    def __init__(self, n_batches, batch, V, H, W, camera="scannet", seed=0, nan_every=0):
        self.n, self.B, self.V, self.H, self.W, self.cam, self.seed, self.nan_every = n_batches, batch, V, H, W, camera, seed, nan_every

    def __len__(self):
        return self.n

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for it in range(self.n):
            rel = synth.make_poses(self.cam, self.B, self.V, g).double()           # ref -> neighbour
            ref_ext = torch.eye(4, dtype=torch.float64).expand(self.B, 4, 4).clone()
            ref_ext[:, :3, 3] = torch.randn(self.B, 3, generator=g, dtype=torch.float64)
            frames = []
            for i in range(self.V + 1):
                ext = ref_ext if i == self.V // 2 else rel[:, i - (i > self.V // 2)] @ ref_ext
                ext = ext.clone()
                if self.nan_every and i == 0 and it % self.nan_every == 0:
                    ext[0] = float("nan")                                           # a lost pose: is_valid must drop the view
                frames.append({"img": torch.rand(self.B, 3, self.H, self.W, generator=g),
                               "gt_dmap": torch.rand(self.B, 1, self.H, self.W, generator=g) * 3 + 1,
                               "extM": ext})
            yield frames, synth.make_intrinsics(self.cam, self.H // 4, self.W // 4, self.B)


class FolderBatches:
    """data.batches(dataset, batch) with a length, which the sharded loop asks for."""

    def __init__(self, dataset, batch):
        self.dataset, self.batch = dataset, batch

    def __len__(self):
        return (len(self.dataset) + self.batch - 1) // self.batch

    def __iter__(self):
        from magnet_amd import data
        return data.batches(self.dataset, self.batch)


def frame_ids(data_array, B):
    """(ref_ids (B), nghbr_ids (V B), view-major as nghbr_imgs) of a loader batch: a frame's id is its (scene_name, img_idx)."""
    ref_dat, nghbr_dats = split_data_array(data_array)
    ids = lambda d: list(zip(d["scene_name"][:B], d["img_idx"][:B]))
    return ids(ref_dat), [fid for d in nghbr_dats for fid in ids(d)]


def run_model(model, runner, data_array, B, ref_img, nghbr_imgs, nghbr_poses, is_valid, cam_intrins):
    """model(...) as test_MaGNet.py:50 calls it, or with `runner` (magnet_amd.sequence.SequenceRunner over the same model) the
    same prediction with every frame's backbones run once."""
    if runner is None:
        return model(ref_img, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, mode="test")
    ref_ids, nghbr_ids = frame_ids(data_array, B)
    return runner.forward(ref_ids, ref_img, nghbr_ids, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, mode="test")


def validate(model, args, test_loader, device, runner=None):
    """The reference's validate() (test_MaGNet.py:27-81), metrics reduced on the device."""
    with torch.no_grad():
        metrics = M.RunningAverageDict()
        for data_array, cam_intrins in test_loader:
            cur_batch_size = data_array[0]["img"].size()[0]
            # relative poses / validity on the device (float64 inverse there; they never come back to the host)
            ref_dat, nghbr_dats, nghbr_poses, is_valid = data_preprocess_device(data_array, cur_batch_size, device)
            ref_img = ref_dat["img"].to(device)
            gt_dmap = ref_dat["gt_dmap"].to(device)
            nghbr_imgs = torch.cat([d["img"].to(device) for d in nghbr_dats], dim=0)       # view-major
            pred_list = run_model(model, runner, data_array, cur_batch_size, ref_img, nghbr_imgs, nghbr_poses, is_valid, cam_intrins)
            crop = "garg" if getattr(args, "garg_crop", False) else ("eigen" if getattr(args, "eigen_crop", False) else None)
            for m in M.compute_depth_errors(pred_list[-1], gt_dmap, args.min_depth, args.max_depth, crop=crop):   # test_MaGNet.py:58-79
                metrics.update(m)
        return metrics.get_value()


def validate_sharded(model, args, test_loader, device, rank=0, world=1, with_count=False, runner=None):
    """validate() over this rank's share of the batches with the metric rows kept on the device (kind='sigma' on pred_list[-1]):
    nothing is read back per batch, and the rows of all ranks are gathered once and averaged in loader order."""
    with torch.no_grad():
        crop = "garg" if getattr(args, "garg_crop", False) else ("eigen" if getattr(args, "eigen_crop", False) else None)
        table = M.MetricTable(device, args.min_depth, args.max_depth, crop=crop, kind="sigma")

        def step(batch):
            data_array, cam_intrins = batch
            cur_batch_size = data_array[0]["img"].size()[0]
            ref_dat, nghbr_dats, nghbr_poses, is_valid = data_preprocess_device(data_array, cur_batch_size, device)
            ref_img = ref_dat["img"].to(device)
            gt_dmap = ref_dat["gt_dmap"].to(device)
            nghbr_imgs = torch.cat([d["img"].to(device) for d in nghbr_dats], dim=0)       # view-major
            pred_list = run_model(model, runner, data_array, cur_batch_size, ref_img, nghbr_imgs, nghbr_poses, is_valid, cam_intrins)
            table.append_pred(pred_list[-1], gt_dmap)

        metrics, n = E.evaluate(step, test_loader, table, rank, world)
        return (metrics, n) if with_count else metrics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8); ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--V", type=int, default=4); ap.add_argument("--D", type=int, default=5); ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--input_height", type=int, default=480); ap.add_argument("--input_width", type=int, default=640)
    ap.add_argument("--min_depth", type=float, default=1e-3); ap.add_argument("--max_depth", type=float, default=10.0)
    ap.add_argument("--feat_dtype", default="fp32"); ap.add_argument("--log", default="")
    ap.add_argument("--dataset_path", default="", help="root of ScanNet-format scene folders (magnet_amd/data.py) instead of synthetic frames")
    ap.add_argument("--split", default="", help="text file of '<scene> <frame index>' lines (data_split/scannet_*.txt format)")
    ap.add_argument("--window_radius", type=int, default=20)
    ap.add_argument("--dataset_format", default="scannet", choices=["scannet", "7scenes"],
                    help="folder layout; the split file has '<scene> <frame>' or '<scene> <sequence> <frame>' lines")
    ap.add_argument("--garg_crop", action="store_true", help="KITTI: evaluate inside the Garg ECCV16 window (test_MaGNet.py:67-68)")
    ap.add_argument("--eigen_crop", action="store_true", help="KITTI: evaluate inside the Eigen NIPS14 window (test_MaGNet.py:69-70)")
    ap.add_argument("--psmnet", action="store_true", help="use the PSMNet F-Net (matrix-core path) instead of the stub F-Net")
    ap.add_argument("--reuse_backbones", action="store_true",
                    help="with --dataset_path: run each frame's backbones once and gather the views of every window from a frame pool "
                         "(magnet_amd/sequence.py); frame ids are the loader's (scene_name, img_idx).  The torch stand-in backbones round differently "
                         "in a batch of another size, so the metrics agree with the default run's to about 7 digits, not to the bit")
    ap.add_argument("--pool_frames", type=int, default=64, help="with --reuse_backbones: frames the pool holds (least recently used go first)")
    ap.add_argument("--graph", action="store_true",
                    help="with --reuse_backbones: replay every step as HIP graphs (SequenceRunner(graph=True)): the same metrics, fewer launches "
                         "from the host; pays when few frames are new per call")
    ap.add_argument("--encoder", default="standin", choices=["standin", "b5"],
                    help="the D-Net: 'standin' (default) is the seeded stub D-Net; 'b5' is the DenseDepth D-Net on the HIP decoder path behind "
                         "the EfficientNet-B5 encoder (magnet_amd/encoder.py), seeded weights unless a checkpoint is loaded by the caller")
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
    if a.graph and not a.reuse_backbones:
        ap.error("--graph is a mode of --reuse_backbones (SequenceRunner(graph=True)): give both")
    if a.reuse_backbones and not a.dataset_path:
        raise SystemExit("--reuse_backbones needs --dataset_path: the synthetic windows share no frames")
    rank, world, device, sharded = E.start(a, __file__)
    from magnet_amd.standin import StubDNet, StubFNet, make_args, seeded_magnet_weights
    args = make_args(D=a.D, iters=a.iters, dpv_h=a.input_height // 4, dpv_w=a.input_width // 4, V=a.V)
    args.min_depth, args.max_depth = a.min_depth, a.max_depth
    args.garg_crop, args.eigen_crop = a.garg_crop, a.eigen_crop
    f_net = StubFNet(2)
    if a.psmnet:
        from magnet_amd.fnet import FNET
        args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
        f_net = FNET(args)                                   # random init unless a checkpoint is loaded by the caller
    if a.encoder == "b5":
        from magnet_amd.standin import make_dnet
        model = MAGNET(args, d_net=make_dnet(backend="hip", encoder="b5", encoder_backend=a.encoder_backend, encoder_precision=a.encoder_precision),
                       f_net=f_net,
                       feat_dtype=a.feat_dtype, dnet_backend="hip")
    else:
        model = MAGNET(args, d_net=StubDNet(1), f_net=f_net, feat_dtype=a.feat_dtype)
    seeded_magnet_weights(model, 3)
    model = model.to(device).eval()
    runner = None
    if a.dataset_path:
        from magnet_amd import data
        with open(a.split) as f:
            samples = [ln.split()[:3 if a.dataset_format == "7scenes" else 2] for ln in f if ln.strip()]
        Folder = data.SevenScenesFolder if a.dataset_format == "7scenes" else data.ScanNetFolder
        ds = Folder(a.dataset_path, samples, n_views=a.V, window_radius=a.window_radius,
                                input_hw=(a.input_height, a.input_width), dpv_hw=(a.input_height // 4, a.input_width // 4),
                                **({"raw_images": True} if a.device_images else {}))
        loader = FolderBatches(ds, a.batch)
        preps = None
        if a.device_images:
            # with a frame pool the frames stay uint8 up to the runner, which prepares only those the pool lacks
            loader, preps = ingest.device_image_loader(a, loader, device, to_runner=a.reuse_backbones)
        if a.reuse_backbones:
            from magnet_amd.sequence import SequenceRunner
            kw = {**({"graph": True} if a.graph else {}), **({"image_prep": preps} if preps is not None else {})}
            runner = SequenceRunner(model, a.pool_frames, **kw)
        title = "scannet-format folder %s (%d windows) V=%d D=%d iters=%d" % (a.dataset_path, len(ds), a.V, a.D, a.iters)
    else:
        loader = SyntheticWindows((a.frames + a.batch - 1) // a.batch, a.batch, a.V, a.input_height, a.input_width, nan_every=3)
        title = "synthetic frames=%d V=%d D=%d iters=%d" % (a.frames, a.V, a.D, a.iters)
    if not sharded:
        M.log_metrics(a.log, validate(model, args, loader, device, runner), title)
        return
    m, n = validate_sharded(model, args, loader, device, rank, world, with_count=True, runner=runner)
    if rank == 0:
        M.log_metrics(a.log, m, title)
        if a.dump_metrics:
            E.dump_metrics(a.dump_metrics, m, n)
    E.finish()


if __name__ == "__main__":
    main()
