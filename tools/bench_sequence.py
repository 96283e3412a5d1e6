"""Sequence inference against MAGNET.forward on one GPU (magnet_amd/sequence.py): C2 and C5 with the matrix-core F-Net and the D-Net
decoder inside the step (stand-in encoder), a sliding window in which every frame is the reference once, neighbours at spacing 1,
B = 8 windows per call.  In one process, after --warmup calls of each, --pairs interleaved pairs of
    MAGNET.forward(windows of call k)   and   SequenceRunner.forward(the same windows)
are timed with HIP events; the runner's pool then holds the frames of the earlier calls, so a call encodes its B new frames.
Prints one JSON line per workload: reference frames/s of both (median over the pairs, and every pair), backbone images encoded per
reference frame, and the gather launch's time and rate (bytes read + written / time).  --out FILE appends the lines.

    python tools/bench_sequence.py [--pairs 8] [--warmup 2] [--configs C2,C5] [--out profiles/sequence/bench_sequence.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--configs", default="C2,C5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from magnet_amd import fnet, lib, synth
    from magnet_amd.magnet import MAGNET
    from magnet_amd.sequence import SequenceRunner
    from magnet_amd.standin import make_args, make_dnet, seeded_magnet_weights
    lib.load()
    dev = torch.device("cuda:0")

    gather_events = []
    real_gather = lib.gather_views

    def timed_gather(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_gather(*args, **kw)
        e1.record()
        gather_events.append((e0, e1))
    lib.gather_views = timed_gather

    for name in a.configs.split(","):
        wl = synth.WORKLOADS[name]
        B, V, h, w = a.batch, wl.V, wl.h, wl.w
        H, W = 4 * h, 4 * w
        args = make_args(D=wl.D, iters=wl.iters, dpv_h=h, dpv_w=w, fdim=64, V=V)
        args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
        model = MAGNET(args, d_net=make_dnet(), f_net=fnet.FNET(args), feat_dtype=wl.feat_dtype, dnet_backend="hip").to(dev).eval()
        seeded_magnet_weights(model, seed=4)
        n_calls = a.warmup + a.pairs
        half = V // 2
        T = n_calls * B + 2 * half
        g = torch.Generator().manual_seed(1)
        frames = torch.rand(T, 3, H, W, generator=g).to(dev)
        offsets = [k for k in range(-half, half + 1) if k != 0]
        runner = SequenceRunner(model, capacity=2 * (B + 2 * half))
        intr = synth.make_intrinsics(wl.camera, h, w, B)
        valid = torch.ones(B, V, dtype=torch.int32)
        pairs, encoded, diffs = [], [], []
        gather_events.clear()
        with torch.no_grad():
            for call in range(n_calls):
                refs = list(range(half + call * B, half + (call + 1) * B))
                nghbrs = [r + o for o in offsets for r in refs]                  # view-major
                ref_img, nghbr_imgs = frames[refs[0]:refs[-1] + 1], torch.cat([frames[refs[0] + o:refs[-1] + 1 + o] for o in offsets])
                poses = synth.make_poses(wl.camera, B, V, g).to(dev)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                want = model(ref_img, nghbr_imgs, poses, valid, intr, mode="test")
                ev[1].record()
                before = runner.encoded
                ev[2].record()
                got = runner.forward(refs, ref_img, nghbrs, nghbr_imgs, poses, valid, intr)
                ev[3].record()
                torch.cuda.synchronize()
                if call >= a.warmup:
                    pairs.append((ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])))
                    encoded.append(runner.encoded - before)
                    diffs.append(float((got[-1] - want[-1]).abs().max()))
        gather_ms = [e0.elapsed_time(e1) for e0, e1 in gather_events[a.warmup:]]
        es = 2 if wl.feat_dtype == "bf16" else 4
        rows = (h + 2) * (w + 2)
        moved = {"x_d3": 2 * B * rows * 256 * 2 * 2, "features": 2 * (V * B * rows + B * h * w) * 64 * es, "gmm": 2 * (1 + V) * B * 2 * h * w * 4}
        gms = statistics.median(gather_ms)
        line = {"bench": "sequence", "config": name, "B": B, "V": V, "D": wl.D, "iters": wl.iters, "feat_dtype": wl.feat_dtype,
                "pairs": len(pairs), "gpu": torch.cuda.get_device_name(0),
                "forward_ms": [round(p[0], 3) for p in pairs], "runner_ms": [round(p[1], 3) for p in pairs],
                "forward_ref_frames_per_s": round(B / statistics.median(p[0] for p in pairs) * 1e3, 1),
                "runner_ref_frames_per_s": round(B / statistics.median(p[1] for p in pairs) * 1e3, 1),
                "runner_faster_in_every_pair": all(p[1] < p[0] for p in pairs),
                "images_encoded_per_ref_frame": {"forward": 1 + V, "runner": sum(encoded) / (len(encoded) * B)},
                "gather_ms": round(gms, 4), "gather_bytes_read_plus_written": moved, "gather_GB_per_s": round(sum(moved.values()) / gms / 1e6, 1),
                "max_abs_diff_last_prediction": max(diffs)}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        del model, runner, frames
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
