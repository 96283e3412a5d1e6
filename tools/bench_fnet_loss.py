"""The tail of the F-Net training step on a synthetic raw volume: the fused pair (magnet_fnet_loss_forward / _backward, csrc/fnet_loss.hip)
against the driver's torch tail (softmax, expected depth, masked L1 and their autograd: tools/bench_train_fnet.py's step from the raw
volume on), alternated in one process and timed with device events, at the reference's training shape (16 frames, D = 80, 120 x 160)
and at B = 4.  Prints one JSON line per batch size: per-pair times, per-kernel time and achieved bytes/s of the fused pair against its
algorithmic bytes (forward 4 BDhw + 12 Bhw, backward 8 BDhw + 12 Bhw) and the 8 TB/s HBM peak, the peak of
torch.cuda.max_memory_allocated for both tails, and the kernels of one torch tail (torch.profiler).

    python tools/bench_fnet_loss.py [--pairs 12] [--warmup 3] [--batches 16 4]
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 4])
    a = ap.parse_args()
    from magnet_amd import lib
    lib.load()
    dev = torch.device("cuda:0")
    D, h, w = 80, 120, 160
    min_depth, max_depth = 0.5, 10.0
    d = torch.linspace(0.25, 8.0, D, device=dev)
    one = torch.ones((), device=dev)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, D, h, w, generator=g) * 3.0).to(dev)
        gt = (torch.rand(B, 1, h, w, generator=g) * 4.5).to(dev)             # about a ninth at or below min_depth
        gt3 = gt[:, 0].contiguous()
        xr = x.clone().requires_grad_(True)

        def fused(times=None):
            e = [ev() for _ in range(3)]
            e[0].record()
            loss, pred, m, rz, sums = lib.fnet_loss_forward(x, d, gt3, min_depth, max_depth)
            e[1].record()
            grad = lib.fnet_loss_backward(x, d, gt3, pred, m, rz, sums, one, min_depth, max_depth)
            e[2].record()
            if times is not None:
                times.append(e)
            return loss, grad

        def torch_tail(times=None):
            xr.grad = None
            e = [ev() for _ in range(2)]
            e[0].record()
            cv = torch.softmax(xr, dim=1)
            pred = torch.sum(cv * d.view(1, D, 1, 1), dim=1, keepdim=True)
            mask = gt > min_depth
            loss = torch.mean(torch.abs(pred[mask] - gt[mask]))
            loss.backward()
            e[1].record()
            if times is not None:
                times.append(e)
            return loss, xr.grad

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
        lf, gf = fused()
        lt, gtor = torch_tail()
        vol, pix = B * D * h * w, B * h * w
        bytes_f, bytes_b = 4 * vol + 12 * pix, 8 * vol + 12 * pix
        med = lambda v: sorted(v)[len(v) // 2]
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            torch_tail()
            torch.cuda.synchronize()
        kern = []
        for e in prof.key_averages():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                t = getattr(e, "device_time_total", None)
                kern.append((e.key[:70], e.count, round((e.cuda_time_total if t is None else t), 1)))
        kern.sort(key=lambda k: -k[2])
        print(json.dumps({
            "shape": dict(B=B, D=D, h=h, w=w), "pairs": a.pairs, "warmup": a.warmup,
            "fused_forward_us": [round(v, 1) for v in fwd], "fused_backward_us": [round(v, 1) for v in bwd], "torch_tail_us": [round(v, 1) for v in tor],
            "fused_faster_in_every_pair": all(f + b < t for f, b, t in zip(fwd, bwd, tor)),
            "median_us": dict(fused_forward=round(med(fwd), 1), fused_backward=round(med(bwd), 1), torch_tail=round(med(tor), 1)),
            "algorithmic_bytes": dict(forward=bytes_f, backward=bytes_b),
            "achieved_TBps": dict(forward=round(bytes_f / med(fwd) / 1e6, 3), backward=round(bytes_b / med(bwd) / 1e6, 3)),
            "share_of_8TBps_hbm_peak": dict(forward=round(bytes_f / med(fwd) * 1e6 / HBM_PEAK, 3), backward=round(bytes_b / med(bwd) * 1e6 / HBM_PEAK, 3)),
            "peak_extra_bytes": peak,
            "loss": dict(fused=float(lf), torch=float(lt)),
            "grad_rel_l2_fused_vs_torch": float((gf.double() - gtor.double()).norm() / gtor.double().norm()),
            "torch_tail_kernels(name, calls, us)": kern[:24], "torch_tail_kernel_launches": sum(k[1] for k in kern),
        }))
        del x, xr, gt, gt3, gf, gtor
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
