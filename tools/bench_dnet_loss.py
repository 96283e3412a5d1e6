"""The tail of the stand-alone D-Net's training step behind the two head convolutions, on synthetic head outputs: the fused pair
(magnet_dnet_loss_forward / _backward, csrc/dnet_loss.hip) against the torch tail (dnet.upsample_depth_via_mask +
gaussian_activation(magnet=False) + the reference's loss expression, under autograd), forward + backward, alternated in pairs in one
process and timed with device events, at (B, h, w) = (4, 120, 160) and (4, 88, 304).  Prints one JSON line per shape: every pair's
times, the fused pair's achieved bytes/s against its algorithmic bytes (forward: the logits once + gt, valid, pred; backward: the
logits and their gradient once + gt, valid + the tap sums written and read) and the 8 TB/s HBM peak, and the peak of
torch.cuda.max_memory_allocated above the inputs for both tails.

    python tools/bench_dnet_loss.py [--pairs 12] [--warmup 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = ((4, 120, 160), (4, 88, 304))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from magnet_amd import dnet, lib
    lib.load()
    dev = torch.device("cuda:0")
    one = torch.ones((), device=dev)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    for B, h, w in SHAPES:
        g = torch.Generator().manual_seed(h)
        depth = (torch.randn(B, 2, h, w, generator=g) * torch.tensor([1.0, 1.5]).view(1, 2, 1, 1) + torch.tensor([2.5, -1.0]).view(1, 2, 1, 1)).to(dev)
        mask = (torch.randn(B, 144, h, w, generator=g) * 3.0).to(dev)
        gt = (torch.rand(B, 1, 4 * h, 4 * w, generator=g) * 5.0 + 0.2).to(dev)
        valid = (torch.rand(B, 1, 4 * h, 4 * w, generator=g) < 0.5).to(dev)
        gt3, valid3 = gt[:, 0].contiguous(), valid[:, 0].contiguous()
        dr, mr = depth.clone().requires_grad_(True), mask.clone().requires_grad_(True)

        def fused(times=None):
            e = [ev() for _ in range(3)]
            e[0].record()
            loss, sums, pred = lib.dnet_loss_forward(depth, mask, gt3, valid3)
            e[1].record()
            gd, gm = lib.dnet_loss_backward(depth, mask, gt3, valid3, sums, one)
            e[2].record()
            if times is not None:
                times.append(e)
            return loss, gd, gm

        def torch_tail(times=None):
            dr.grad = mr.grad = None
            e = [ev() for _ in range(2)]
            e[0].record()
            pred = dnet.gaussian_activation(dnet.upsample_depth_via_mask(dr, mr, 4), magnet=False)
            gts = gt[valid]                                                  # utils/losses.py:15-22
            mu, var = torch.split(pred, 1, dim=1)
            mu = mu[valid]
            var = var[valid]
            var[var < 1e-10] = 1e-10
            loss = torch.mean((torch.square(mu - gts) / (2 * var)) + (0.5 * torch.log(var)))
            loss.backward()
            e[1].record()
            if times is not None:
                times.append(e)
            return loss, dr.grad, mr.grad

        peak = {}
        for name, fn in (("fused", fused), ("torch", torch_tail)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
            del out
        tf, tt = [], []
        for _ in range(a.pairs):
            fused(tf)
            torch_tail(tt)
        torch.cuda.synchronize()
        fwd = [e[0].elapsed_time(e[1]) * 1e3 for e in tf]
        bwd = [e[1].elapsed_time(e[2]) * 1e3 for e in tf]
        tor = [e[0].elapsed_time(e[1]) * 1e3 for e in tt]
        lf, gdf, gmf = fused()
        lt, gdt, gmt = torch_tail()
        pix = B * h * w
        bytes_f = pix * (144 * 4 + 16 * (4 + 1 + 8))                         # logits + gt + valid + pred per coarse pixel
        bytes_b = pix * (2 * 144 * 4 + 16 * (4 + 1) + 2 * 18 * 4 + 8)       # logits, their gradient, gt, valid, tap sums out and in, grad_depth
        med = lambda v: sorted(v)[len(v) // 2]
        rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
        print(json.dumps({
            "shape": dict(B=B, h=h, w=w), "pairs": a.pairs, "warmup": a.warmup,
            "fused_forward_us": [round(v, 1) for v in fwd], "fused_backward_us": [round(v, 1) for v in bwd], "torch_tail_us": [round(v, 1) for v in tor],
            "fused_faster_in_every_pair": all(f + b < t for f, b, t in zip(fwd, bwd, tor)),
            "median_us": dict(fused_forward=round(med(fwd), 1), fused_backward=round(med(bwd), 1), torch_tail=round(med(tor), 1)),
            "algorithmic_bytes": dict(forward=bytes_f, backward=bytes_b),
            "achieved_TBps": dict(forward=round(bytes_f / med(fwd) / 1e6, 3), backward=round(bytes_b / med(bwd) / 1e6, 3)),
            "share_of_8TBps_hbm_peak": dict(forward=round(bytes_f / med(fwd) * 1e6 / HBM_PEAK, 3), backward=round(bytes_b / med(bwd) * 1e6 / HBM_PEAK, 3)),
            "peak_extra_bytes": peak,
            "loss": dict(fused=float(lf), torch=float(lt.detach())),
            "grad_rel_l2_fused_vs_torch": dict(depth=rel(gdf, gdt), mask=rel(gmf, gmt)),
        }))
        del depth, mask, gt, valid, dr, mr, gdf, gmf, gdt, gmt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
