#!/usr/bin/env python3
"""Dev tool (GPU box): time the fused cost-volume kernel alone under kernel selection / dev switches (`path`).
usage: python tools/ablate.py [workload] [frames] [split]      (split: time the split-bf16 channel-last output form)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from magnet_amd import synth, lib
lib.use_dev_build()
from magnet_amd.homography import CostVolumeCW
from magnet_amd.magnet import depth_sampling
from bench import device_inputs

wl = synth.WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "C2"]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
split = len(sys.argv) > 3 and sys.argv[3] == "split"
dev = torch.device("cuda:0")
inp = device_inputs(wl, B, 1000, dev)
if os.environ.get("ABLATE_SMOOTH"):                      # smooth synthetic variant (synth.make_inputs smooth=): low-passed features and (mu, sigma) maps
    sm = synth.make_inputs(wl, B=B, seed=1000, smooth=int(os.environ["ABLATE_SMOOTH"]), round_bf16=(wl.feat_dtype == "bf16"))
    for k_ in ("ref_feat", "nghbr_feat", "ref_gmms", "nghbr_gmms"):
        inp[k_] = sm[k_].to(dev)
k = depth_sampling(3, wl.D)
out = torch.empty(B, wl.D, wl.h, wl.w, device=dev)
ld = (wl.D + 7) // 8 * 8 + 256
hi = torch.zeros(B * (wl.h + 2) * (wl.w + 2), ld, dtype=torch.bfloat16, device=dev); lo = torch.zeros_like(hi)
fdt = wl.feat_dtype
# needs a dev build of the library (python -m magnet_amd.build --dev): bits 8.. of `path` travel as MagnetCostVolumeArgs.dev_flags.
# Every dev flag only routes the launch to another kernel that the product library ships too.
R2 = 0x100 << 8                                       # dev flag 0x100: the round-2 production kernels although the quad map is given
PV = 0x900 << 8                                       # + 0x800: the per-view kernel (cost_volume_fast.hip) instead of the batched-view one
IF = 0x400 << 8                                       # dev flag 0x400: cost_volume_fast64.hip's other item form (bf16: quad items, fp32: texel pairs)
VARIANTS = [("production (auto)", 0), ("round-2 kernel (fast64)", 4 | R2), ("round-2 kernel, other item form", 4 | R2 | IF),
            ("per-view kernel (fast)", 4 | PV), ("exact cand", 2), ("production (auto), again", 0)]
if os.environ.get("ABLATE_SHORT"):
    VARIANTS = VARIANTS[:2]
for name, path in VARIANTS:
    if split and (path & 0xff) == 3:
        continue
    cv = CostVolumeCW(inp["ref_feat"], inp["nghbr_feat"], inp["nghbr_gmms"], inp["nghbr_poses"], inp["is_valid"],
                      inp["cam_intrins"], 5, feat_dtype=fdt, path=path)
    kw = dict(out_split=(hi, lo, ld)) if split else dict(out=out)
    try:
        cv(ref_gmm=inp["ref_gmms"], k_list=k, **kw)
    except lib.MagnetError as e:
        print(f"{wl.name} {name}: {e}"); continue
    # the chip's clock / power state drifts for the first second of load (20-launch samples differed by 8 % between the first and
    # the last variant of one process): ~0.3 s of the same kernel first, then the median of 5 samples of 40 launches
    for _ in range(300):
        cv(ref_gmm=inp["ref_gmms"], k_list=k, **kw)
    torch.cuda.synchronize()
    n, samples = 40, []
    for _ in range(5):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            cv(ref_gmm=inp["ref_gmms"], k_list=k, **kw)
        e1.record(); torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) / n)
    ms = sorted(samples)[2]
    gbs = wl.algorithmic_bytes() * B / (ms * 1e-3) / 1e9
    print(f"{wl.name} B={B} {fdt:5s} {'split' if split else 'nchw '} {name:30s}: {ms:8.3f} ms/launch (5 samples {min(samples):.3f}..{max(samples):.3f})  alg {gbs:7.1f} GB/s = {gbs / 80:5.1f} % of 8 TB/s")
