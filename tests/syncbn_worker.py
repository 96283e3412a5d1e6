"""One rank of tests/test_gpu_fnet_syncbn.py's two-rank runs (not a test module).  Started once per rank with RANK / WORLD_SIZE /
MASTER_ADDR / MASTER_PORT in the environment:

    python tests/syncbn_worker.py --backend gloo|nccl --out DIR --cases even,uneven,ddp

gloo: both ranks share cuda:0 (a correctness vehicle); nccl: rank r runs on cuda:r.  The process-group timeout is 60 s, and a rank
that raises prints its traceback and exits non-zero at once, so the launcher can stop its partner.  Each case writes
DIR/<case>_rank<r>.npz.  The inputs of every case are built here, from seeds, for the test process to rebuild in whole."""
import argparse
import copy
import datetime
import os
import sys
import traceback

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHARDS = {"even": (1, 1), "uneven": (2, 1)}                       # images of 256 x 256 per rank
H = W = 256
FDIM = 32
DDP_D = 32


def fnet_base():
    from magnet_amd import fnet
    from tests.stubs import seeded_fnet_state
    return seeded_fnet_state(fnet.PSMNet(feature_dim=FDIM), seed=3).train()


def images(N):
    from tests.stubs import procedural_images
    img = procedural_images(N, H, W)
    return img + 0.05 * torch.randn(img.shape, generator=torch.Generator().manual_seed(N * 7 + H))


def feature_gradient(N):
    return torch.randn(N, FDIM, H // 4, W // 4, generator=torch.Generator().manual_seed(17))


def shard(case, rank):
    """[lo, hi): the images of `case` that `rank` holds."""
    sizes = SHARDS[case]
    lo = sum(sizes[:rank])
    return lo, lo + sizes[rank]


def bn_buffers(psm):
    return {k: v.detach().cpu().numpy() for k, v in psm.state_dict().items() if "running" in k or "num_batches" in k}


def ddp_case():
    """MAGNET_F at B = 2 reference frames, V = 1 source view each, 256 x 256 -> a 64 x 64 grid, D = 32 bins, and the weights of
    the sum-form loss over the raw volume.  Rank r of the DDP run takes frame r (B = 1)."""
    from magnet_amd import synth
    from magnet_amd.standin import make_args
    args = make_args(D=DDP_D, iters=1, dpv_h=H // 4, dpv_w=W // 4, fdim=FDIM, V=1)
    args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", FDIM
    gen = torch.Generator().manual_seed(29)
    img = images(4)
    ref_img, nb = img[:2], img[2:]
    poses = synth.make_poses("scannet", 2, 1, gen)
    valid = torch.ones(2, 1, dtype=torch.int32)
    cam = synth.make_intrinsics("scannet", H // 4, W // 4, 2)
    d_center = torch.linspace(0.5, 6.0, DDP_D).view(1, -1, 1, 1)
    w = torch.randn(2, DDP_D, H // 4, W // 4, generator=gen)
    return args, ref_img, nb, poses, valid, cam, d_center, w


def ddp_fnet(args):
    from magnet_amd import fnet
    from tests.stubs import seeded_fnet_state
    return seeded_fnet_state(fnet.FNET(args), seed=7)


def ddp_loss(m, case, lo, hi, dev):
    args, ref_img, nb, poses, valid, cam, d_center, w = case
    vol = m(ref_img[lo:hi].to(dev), nb[lo:hi].to(dev), poses[lo:hi].to(dev), valid[lo:hi].to(dev),
            {k: v[lo:hi].to(dev) for k, v in cam.items() if torch.is_tensor(v)}, d_center, softmax=False)
    return (vol * w[lo:hi].to(dev)).sum()


def _grads(m):
    return {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}


def run_fnet(case, rank, dev, out):
    from magnet_amd.train_fnet import FNetTrainHIP, fnet_train_hip
    n_all = sum(SHARDS[case])
    lo, hi = shard(case, rank)
    img, gfeat = images(n_all)[lo:hi].to(dev), feature_gradient(n_all)[lo:hi].to(dev)
    steps = []
    for _ in range(2):                                               # the same step twice, from the same state
        psm = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(fnet_base())).to(dev).train()
        feat = fnet_train_hip(FNetTrainHIP(psm), img)
        (feat * gfeat).sum().backward()
        steps.append((feat.detach().cpu().numpy(), _grads(psm), bn_buffers(psm)))
    (f0, g0, b0), (f1, g1, b1) = steps
    repeat = np.array_equal(f0, f1) and all(np.array_equal(g0[k], g1[k]) for k in g0) and all(np.array_equal(b0[k], b1[k]) for k in b0)
    np.savez(os.path.join(out, f"{case}_rank{rank}.npz"), feat=f0, repeat=np.array(repeat),
             **{"grad:" + k: v for k, v in g0.items()}, **{"buf:" + k: v for k, v in b0.items()})


def run_ddp(rank, dev, out):
    from torch.nn.parallel import DistributedDataParallel
    from magnet_amd.magnet import MAGNET_F
    case = ddp_case()
    m = MAGNET_F(case[0], ddp_fnet(case[0]), train_backend="hip")
    m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m).to(dev).train()
    ddp = DistributedDataParallel(m, device_ids=[dev.index])
    opt = torch.optim.AdamW(ddp.parameters(), lr=3.57e-4, weight_decay=0.01)
    ddp_loss(ddp, case, rank, rank + 1, dev).backward()
    grads = _grads(m)
    opt.step()
    np.savez(os.path.join(out, f"ddp_rank{rank}.npz"), **{"grad:" + k: v for k, v in grads.items()},
             **{"param:" + k: p.detach().cpu().numpy() for k, p in m.named_parameters()}, **{"buf:" + k: v for k, v in bn_buffers(m).items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", required=True, choices=("gloo", "nccl"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", required=True)
    a = ap.parse_args()
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", rank if a.backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    kw = {"device_id": dev} if a.backend == "nccl" else {}
    dist.init_process_group(a.backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60), **kw)
    for case in a.cases.split(","):
        if case == "ddp":
            run_ddp(rank, dev, a.out)
        else:
            run_fnet(case, rank, dev, a.out)
    torch.cuda.synchronize()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
