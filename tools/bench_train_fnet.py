"""Timing of one MAGNET_F training step of train_FNet.py (lines 69-119): the F-Net on the B(1+V) images in .train() mode, est_costvolume_F,
the L1 loss on the expected depth, and the backward, for train_backend 'torch' (nn.Conv2d / BatchNorm2d under autograd) and 'hip'
(magnet_amd/train_fnet.py), at 480 x 640, V = 4, D = 80, F = 64, B = 1 (the ScanNet config per GPU) and B = 4 (the driver's default).
--loss torch (default) runs the driver's own tail (softmax in est_costvolume_F, expected depth and masked L1 as torch ops); --loss hip takes the
raw volume and magnet_amd.losses.FnetLoss (the fused tail, csrc/fnet_loss.hip).
Also times the no-grad training-mode forward.  Prints one JSON line: ms_per_train_step and ms_per_train_forward per backend and batch,
and the time per kernel of the HIP step (torch.profiler) at B = 4.

    python tools/bench_train_fnet.py [--steps 10] [--warmup 3] [--loss {torch,hip}]
    python tools/bench_train_fnet.py --gpus N [--dist_backend {nccl,gloo}]

--gpus N (or a launcher's RANK / WORLD_SIZE) times the reference's multi-GPU step instead (train_FNet.py:220-222): every rank
converts the F-Net with nn.SyncBatchNorm.convert_sync_batchnorm, wraps MAGNET_F in DistributedDataParallel and steps on its own B
frames; each step time is the slowest rank's.  'hip' is then the synchronised HIP path, 'torch' nn.SyncBatchNorm under autograd.  The
kernel profile is skipped.  gloo lets ranks share a GPU: a correctness vehicle, not a timing.
"""
import argparse
import copy
import json
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss", default="torch", choices=["torch", "hip"], help="the tail of the step: torch ops (the driver's) or FnetLoss")
    ap.add_argument("--gpus", type=int, default=1, help="start this many ranks of this command line (dist.spawn_ranks): the DDP + SyncBatchNorm step")
    ap.add_argument("--dist_backend", default="nccl", choices=["nccl", "gloo"], help="process-group backend; gloo lets several ranks share one GPU")
    a = ap.parse_args()
    from magnet_amd import dist as mdist
    launched = "RANK" in os.environ
    if a.gpus > 1 and not launched:
        raise SystemExit(mdist.spawn_ranks(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))
    rank, world, local = mdist.env_world() if launched else (0, 1, 0)
    n_dev = torch.cuda.device_count()
    if launched:
        if a.dist_backend == "nccl" and world > n_dev:
            raise SystemExit(f"{world} ranks on {n_dev} GPU(s): nccl needs one GPU per rank; use --dist_backend gloo to share GPUs")
        mdist.init_from_env(backend=a.dist_backend)
    from magnet_amd import fnet, lib, synth
    from magnet_amd.losses import FnetLoss
    from magnet_amd.magnet import MAGNET_F
    from magnet_amd.train_fnet import FNetTrainHIP
    lib.load()
    dev = torch.device("cuda", local % n_dev)
    torch.cuda.set_device(dev)
    V, H, W, F, D = 4, 480, 640, 64, 80
    args = SimpleNamespace(FNET_architecture="PSM-Net", FNET_feature_dim=F)
    torch.manual_seed(0)
    base = fnet.FNET(args).train()
    d_center = torch.linspace(0.25, 8.0, D).view(1, -1, 1, 1)
    fnet_loss = FnetLoss(SimpleNamespace(loss_fn="l1", min_depth=0.5, max_depth=10.0))
    res = {"config": dict(V=V, H=H, W=W, F=F, D=D), "ranks": world, "dist_backend": a.dist_backend if world > 1 else None, "loss": a.loss, "steps": a.steps, "warmup": a.warmup, "ms_per_train_step": {},
           "ms_per_train_forward": {}}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return round(mdist.max_over_ranks((time.perf_counter() - t0) * 1e3 / a.steps, device=dev), 3)

    for B in (1, 4):
        gen = torch.Generator().manual_seed(B + 100 * rank)
        ref_img = torch.rand(B, 3, H, W, generator=gen).to(dev)
        nb = torch.rand(V * B, 3, H, W, generator=gen).to(dev)
        poses = synth.make_poses("scannet", B, V, gen).to(dev)
        valid = torch.ones(B, V, dtype=torch.int32, device=dev)
        cam = {k: v.to(dev) for k, v in synth.make_intrinsics("scannet", H // 4, W // 4, B).items()}
        gt = (1.0 + 3.0 * torch.rand(B, 1, H // 4, W // 4, generator=gen)).to(dev)
        for backend in ("torch", "hip"):
            m = MAGNET_F(args, copy.deepcopy(base), train_backend=backend).to(dev).train()
            model = m
            if world > 1:
                m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
                model = torch.nn.parallel.DistributedDataParallel(m, device_ids=[dev.index])

            def step():
                m.zero_grad(set_to_none=True)
                if a.loss == "hip":
                    fnet_loss(model(ref_img, nb, poses, valid, cam, d_center, softmax=False), d_center, gt).backward()
                    return
                cv = model(ref_img, nb, poses, valid, cam, d_center)
                pred = torch.sum(cv * d_center.to(dev), dim=1, keepdim=True)
                mask = gt > 0.5
                torch.mean(torch.abs(pred[mask] - gt[mask])).backward()

            res["ms_per_train_step"][f"{backend}_B{B}"] = timed(step)
            imgs = torch.cat((ref_img, nb))
            psm = m.f_net.f_net
            fwd = psm if backend == "torch" else FNetTrainHIP(psm).run
            with torch.no_grad():
                res["ms_per_train_forward"][f"{backend}_B{B}"] = timed(lambda: fwd(imgs))
            if backend == "hip" and B == 4 and world == 1:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    step()
                    torch.cuda.synchronize()
                per = {}
                for e in prof.key_averages():
                    if e.device_type == torch.autograd.DeviceType.CUDA:
                        t = getattr(e, "device_time_total", None)
                        if t is None:
                            t = e.cuda_time_total
                        per[e.key[:80]] = round(per.get(e.key[:80], 0.0) + t / 1e3, 3)
                res["hip_step_kernels_ms_B4"] = dict(sorted(per.items(), key=lambda kv: -kv[1])[:16])
            del m, model, fwd, psm
            torch.cuda.empty_cache()
    if rank == 0:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
