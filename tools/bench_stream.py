"""Streaming inference, eager against replayed (magnet_amd/sequence.py, SequenceRunner(graph=True)): one process, B = 1, V = 4, a causal
window (reference frame t - 2, views t - 4, t - 3, t - 1, t), one new frame per step; the matrix-core F-Net, the HIP D-Net decoder and
the stand-in encoder are inside the step.  Two runners over ONE model, graph=False and graph=True, take the same frames: both run the
same kernels of the same build, so the eager side of a pair is the comparison.  After --warmup steps of each, --pairs interleaved
pairs are timed twice with a host clock around work that ends in a device synchronise (at one frame the host is what a step waits
for, so the host's time is the step's): once per whole step (add + refine, one synchronise at its end) and once split (a synchronise
behind add and one behind refine).  Prints one JSON line per workload: ms per step of both sides (median and every pair), how many
pairs each side wins, the add / refine split, and at C2 the scatter launch's time and rate (bytes read + written / time, HIP events
around 20 launches).  --out FILE appends the lines.

    python tools/bench_stream.py [--pairs 12] [--warmup 3] [--configs C2,shipped,C4] [--out profiles/stream/bench_stream.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402

FP16 = dict(conv_precision="fp16", fnet_precision="fp16", dnet_precision="fp16", dnet_split_k="auto")
OFFSETS = (-2, -1, 1, 2)                       # views of the window centred on t - 2: frames t - 4, t - 3, t - 1, t


def clock(fn):
    """Host milliseconds of fn() up to the device having finished it."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="C2,shipped,C4", help="names of magnet_amd.synth.WORKLOADS (C4: KITTI, 352x1216 images); V is 4 throughout")
    ap.add_argument("--precisions", default="default,fp16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from magnet_amd import fnet, lib, synth
    from magnet_amd.magnet import MAGNET
    from magnet_amd.sequence import SequenceRunner
    from magnet_amd.standin import make_args, make_dnet, seeded_magnet_weights
    lib.load()
    dev = torch.device("cuda:0")

    for name in a.configs.split(","):
        wl = synth.WORKLOADS[name]
        h, w, V = wl.h, wl.w, 4
        H, W = 4 * h, 4 * w
        for prec in a.precisions.split(","):
            kw = FP16 if prec == "fp16" else {}
            args = make_args(D=wl.D, iters=wl.iters, dpv_h=h, dpv_w=w, fdim=64, V=V)
            args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
            d = make_dnet(backend="hip", split_k=kw.get("dnet_split_k", 0), precision=kw.get("dnet_precision", "bf16x3"))
            model = MAGNET(args, d_net=d, f_net=fnet.FNET(args), feat_dtype=wl.feat_dtype, dnet_backend="hip", **kw).to(dev).eval()
            seeded_magnet_weights(model, seed=4)
            n_steps = a.warmup + 2 * a.pairs
            g = torch.Generator().manual_seed(1)
            frames = torch.rand(4 + n_steps, 3, H, W, generator=g).to(dev)
            runners = {"eager": SequenceRunner(model, 8), "graph": SequenceRunner(model, 8, graph=True)}
            intr = synth.make_intrinsics(wl.camera, h, w, 1)
            valid = torch.ones(1, V, dtype=torch.int32)
            whole = {k: [] for k in runners}
            split = {k: [] for k in runners}
            diffs = []
            with torch.no_grad():
                for r in runners.values():
                    r.add(list(range(4)), frames[:4])
                for step in range(n_steps):
                    t = 4 + step
                    refs, nghbrs = [t - 2], [t - 2 + o for o in OFFSETS]
                    poses = synth.make_poses(wl.camera, 1, V, g).to(dev)
                    timed, parts = step >= a.warmup, step >= a.warmup and (step - a.warmup) % 2 == 1
                    outs = {}
                    order = ("eager", "graph") if step % 4 < 2 else ("graph", "eager")     # neither side always goes first
                    for k in order:
                        r = runners[k]
                        if parts:
                            ms_add, _ = clock(lambda: r.add([t], frames[t:t + 1]))
                            ms_ref, outs[k] = clock(lambda: r.refine(refs, nghbrs, poses, valid, intr))
                            split[k].append((ms_add, ms_ref))
                        else:
                            ms, outs[k] = clock(lambda: (r.add([t], frames[t:t + 1]), r.refine(refs, nghbrs, poses, valid, intr))[1])
                            if timed:
                                whole[k].append(ms)
                    diffs.append(float((outs["eager"][-1] - outs["graph"][-1]).abs().max()))
            med = statistics.median
            pairs = list(zip(whole["eager"], whole["graph"]))
            line = {"bench": "stream", "config": name, "precision": prec, "image": [H, W], "B": 1, "V": V, "D": wl.D, "iters": wl.iters,
                    "feat_dtype": wl.feat_dtype, "pairs": len(pairs), "gpu": torch.cuda.get_device_name(0),
                    "eager_ms": [round(p[0], 3) for p in pairs], "graph_ms": [round(p[1], 3) for p in pairs],
                    "eager_ms_median": round(med(whole["eager"]), 3), "graph_ms_median": round(med(whole["graph"]), 3),
                    "pairs_won": {"eager": sum(p[0] < p[1] for p in pairs), "graph": sum(p[1] < p[0] for p in pairs)},
                    "add_ms_median": {k: round(med(s[0] for s in split[k]), 3) for k in runners},
                    "refine_ms_median": {k: round(med(s[1] for s in split[k]), 3) for k in runners},
                    "add_ms": {k: [round(s[0], 3) for s in split[k]] for k in runners},
                    "refine_ms": {k: [round(s[1], 3) for s in split[k]] for k in runners},
                    "graph_stats": {kind: {str(k): v for k, v in d_.items()} for kind, d_ in runners["graph"].graph_stats.items()},
                    "max_abs_diff_last_prediction": max(diffs)}
            if name == "C2" and prec == "default":
                line.update(scatter_rate(runners["graph"], lib))
            print(json.dumps(line), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")
            del model, runners, frames
            torch.cuda.empty_cache()


def scatter_rate(runner, lib, launches=20):
    """One frame's scatter into the runner's pool, from buffers of the staged shapes: the time of one launch (HIP events around
    `launches` of them) and the bytes read plus written over it."""
    pool = runner.pool
    rows = (pool.h + 2) * (pool.w + 2)
    feat = torch.zeros((1,) + tuple(pool.feat.shape[1:]), dtype=pool.feat.dtype, device=pool.device)
    gmm = torch.zeros((1, 2, pool.h, pool.w), device=pool.device)
    hi, lo = (torch.zeros((rows, 256), dtype=torch.bfloat16, device=pool.device) for _ in range(2))
    slots = torch.tensor([3], dtype=torch.int32, device=pool.device)
    scratch = [torch.zeros_like(t) for t in (pool.feat, pool.gmm, pool.xd3_hi, pool.xd3_lo)]     # a pool of the same shape: the runner's stays as it is
    run = lambda: lib.scatter_frames(slots, pool_feat=scratch[0], pool_gmm=scratch[1], pool_xd3=(scratch[2], scratch[3]), feat=feat, gmm=gmm, xd3=(hi, lo))
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / launches
    moved = 2 * sum(t.numel() * t.element_size() for t in (feat, gmm, hi, lo))
    return {"scatter_ms": round(ms, 4), "scatter_bytes_read_plus_written": moved, "scatter_GB_per_s": round(moved / ms / 1e6, 1)}


if __name__ == "__main__":
    main()
