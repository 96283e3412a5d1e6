"""Training-step timing of MAGNET at the reference's training configuration (train_scripts/magnet/scannet.txt: B = 4, 480 x 640
images -> 120 x 160 grid, V = 4, D = 5, I = 3, gamma 0.8): forward mode='train' + MagnetLoss + backward, for train_backend 'torch'
and 'hip'.  The backbones are stand-ins whose outputs are precomputed (a cached lookup), so only matcher + heads + loss are timed.
Prints one JSON line: ms_per_train_step per backend and the time per backward kernel of the HIP path (torch.profiler).

    python tools/bench_train.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


class _Cached(nn.Module):
    """Returns the precomputed output of a backbone (no compute inside the timed step)."""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from magnet_amd import lib, synth
    from magnet_amd.losses import MagnetLoss
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import StubDNet, StubFNet, make_args, seeded_magnet_weights
    lib.load()
    dev = torch.device("cuda:0")
    B, V, h, w, D, I = 4, 4, 120, 160, 5, 3
    args = make_args(D=D, iters=I, dpv_h=h, dpv_w=w)
    gen = torch.Generator().manual_seed(0)
    ref_img = torch.rand(B, 3, 4 * h, 4 * w, generator=gen).to(dev)
    nb = torch.rand(V * B, 3, 4 * h, 4 * w, generator=gen).to(dev)
    poses = synth.make_poses("scannet", B, V, gen).to(dev)
    valid = torch.ones(B, V, dtype=torch.int32)
    intr = synth.make_intrinsics("scannet", h, w, B)
    gt = (torch.rand(B, 1, 4 * h, 4 * w, generator=gen) * 3 + 1).to(dev)
    gmask = (torch.rand(B, 1, 4 * h, 4 * w, generator=gen) > 0.2).to(dev)
    with torch.no_grad():
        dnet_out = tuple(t.to(dev) for t in StubDNet(seed=21).to(dev)(torch.cat((ref_img, nb), 0)))
        fnet_out = StubFNet(seed=22, fdim=64).to(dev)(torch.cat((ref_img, nb), 0))
    crit = MagnetLoss(SimpleNamespace(loss_fn="gaussian", loss_gamma=0.8))
    res = {"config": dict(B=B, V=V, h=h, w=w, D=D, I=I, F=64), "steps": a.steps, "warmup": a.warmup}
    for backend in ("torch", "hip"):
        m = MAGNET(args, d_net=_Cached(dnet_out), f_net=_Cached(fnet_out), train_backend=backend)
        seeded_magnet_weights(m, seed=23, gain=0.25)
        m = m.to(dev).train()

        def step():
            m.zero_grad(set_to_none=True)
            preds = m(ref_img, nb, poses, valid, intr, mode="train")
            crit(preds, gt, gmask).backward()
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        res[f"ms_per_train_step_{backend}"] = round((time.perf_counter() - t0) * 1e3 / a.steps, 3)
        if backend == "hip":
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    step()
                    torch.cuda.synchronize()
                k = {}
                for ev in prof.key_averages():
                    name = ev.key
                    for tag in ("nll_partial", "nll_final", "nll_backward", "upbwd_pixel", "upbwd_gather", "dgrad_kernel", "wgrad_kernel",
                                "wgrad_bias", "wgrad_reduce", "conv_mfma"):
                        if tag in name:
                            t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                            k[tag] = round(k.get(tag, 0) + t / 1e3, 3)
                res["hip_kernel_ms_per_step"] = k
            except Exception as e:  # the profiler is optional: the step time above stands on its own
                res["hip_kernel_ms_per_step"] = f"profiler unavailable: {type(e).__name__}"
        del m
        torch.cuda.empty_cache()
    res["hip_speedup"] = round(res["ms_per_train_step_torch"] / res["ms_per_train_step_hip"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
