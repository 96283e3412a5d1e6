#!/usr/bin/env python
"""Latency mode A/B in one process: the stacks' 3x3 launches as 128-row tiles (ConvStackMFMA.small_tiles = False) against 64-row tiles
(True) at 1, 2, 3, 4 and 8 frames per step, interleaved pairs, HIP events around the whole match_and_refine and (through
ConvStackMFMA.event_sink, plus a bracket around the hoisted invariant launch) around each 3x3 launch.

    python tools/bench_latency.py [--workloads shipped,C2,C4] [--frames 1,2,3,4,8] [--pairs 12] [--out profiles/latency/bench_latency.jsonl]

Then the step of either form captured as a HIP graph and replayed (20 replays per sample): the step's device time without the host.

One JSON line per (workload, frames): median step (eager: step_ms, replayed: replay_ms) and launch times of either form, and in how
many pairs the 64-row form was faster (the sign test that decides convnet.SMALL_TILE_LIMIT: all pairs or not at all).  One more line: MAGNET.forward's wall time at one frame
with the stand-in backbones.  The outputs of the two forms are compared with torch.equal on the way."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402
from magnet_amd import convnet, lib, synth  # noqa: E402
from magnet_amd.convnet import ConvStackMFMA  # noqa: E402
from magnet_amd.magnet import MAGNET  # noqa: E402


def _ms(pairs):
    return [s.elapsed_time(e) for s, e in pairs]


def measure(wl_name, B, n_pairs, warmup, dev):
    wl = synth.WORKLOADS[wl_name]
    model = MAGNET(bench.make_args(wl, wl.iters), d_net=bench._NoBackbone(), f_net=bench._NoBackbone(), feat_dtype=wl.feat_dtype).to(dev).eval()
    inp = bench.device_inputs(wl, B, seed=1000, device=dev)
    inv_events = []
    plain_invariant = ConvStackMFMA.run_invariant

    def run_invariant(self, *a, **k):                     # the once-per-forward x_d3 launch is not in event_sink: bracket it here
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = plain_invariant(self, *a, **k)
        e.record()
        inv_events.append((s, e))
        return out

    def step(mode, timed):
        ConvStackMFMA.small_tiles = mode
        ConvStackMFMA.event_sink = sink = [] if timed else None
        del inv_events[:]
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            s.record()
            out = model.match_and_refine(inp["ref_gmms"], inp["x_d3"], inp["ref_feat"], inp["nghbr_feat"], inp["nghbr_gmms"],
                                         inp["nghbr_poses"], inp["is_valid"], inp["cam_intrins"], mode="test")
            e.record()
        torch.cuda.synchronize()
        ConvStackMFMA.event_sink = None
        if not timed:
            return out, None
        launches = _ms(inv_events) + _ms([(x[0], x[1]) for x in sink if x[3] == 9])
        return out, dict(step=s.elapsed_time(e), launches=launches)

    ConvStackMFMA.run_invariant = run_invariant
    try:
        outs = {}
        for mode in (False, True):
            for _ in range(warmup):
                outs[mode] = [o.clone() for o in step(mode, False)[0]]
        identical = all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))
        g_stack, m_stack = model._stacks
        tiles = {}
        ConvStackMFMA.record_tiles = True                      # one untimed step per form: what the library says it launched
        for mode in (False, True):
            step(mode, False)
            tiles[mode] = [list(t) for t in list(g_stack.last_invariant_tiles if wl.iters >= 2 else []) + list(g_stack.last_tiles) + list(m_stack.last_tiles)]
        ConvStackMFMA.record_tiles = False
        rec = {False: [], True: []}
        for i in range(n_pairs):
            for mode in ((False, True) if i % 2 == 0 else (True, False)):      # alternate who goes first
                rec[mode].append(step(mode, True)[1])
        # the same step captured once per form and REPLAYED (magnet_amd/graph.py): the host is out of the loop, so this is the
        # step's device time — eagerly launched, a one-frame step waits for the host between its kernels
        from magnet_amd.graph import GraphedRefine
        ConvStackMFMA.run_invariant = plain_invariant         # no timing events inside a capture
        graphs = {}
        for mode in (False, True):
            ConvStackMFMA.small_tiles = mode
            graphs[mode] = GraphedRefine(model, inp["ref_gmms"], inp["x_d3"], inp["ref_feat"], inp["nghbr_feat"], inp["nghbr_gmms"],
                                         inp["nghbr_poses"], inp["is_valid"], inp["cam_intrins"], mode="test")

        def replay(mode, reps=20):
            g = graphs[mode]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                out = g(*g.static)
            e.record()
            torch.cuda.synchronize()
            return out, s.elapsed_time(e) / reps

        for mode in (False, True):
            outs[mode] = [o.clone() for o in replay(mode)[0]]
        identical = identical and all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))
        rep = {False: [], True: []}
        for i in range(n_pairs):
            for mode in ((False, True) if i % 2 == 0 else (True, False)):
                rep[mode].append(replay(mode)[1])
        del graphs
    finally:
        ConvStackMFMA.run_invariant = plain_invariant
        ConvStackMFMA.small_tiles = "auto"
        ConvStackMFMA.record_tiles = False
    med = statistics.median
    n_launch = len(rec[False][0]["launches"])
    line = dict(kind="match_and_refine", workload=wl_name, frames=B, iters=wl.iters, D=wl.D, grid=[wl.h, wl.w], pairs=n_pairs,
                tiles128=convnet.tiles_128(B, wl.h, wl.w + 2), identical=identical,
                last_tiles={"bm128": tiles[False], "bm64": tiles[True]},
                replay_ms={"bm128": round(med(rep[False]), 4), "bm64": round(med(rep[True]), 4)},
                replay_pairs_bm64_faster=sum(b < a for a, b in zip(rep[False], rep[True])),
                step_ms={"bm128": round(med(r["step"] for r in rec[False]), 4), "bm64": round(med(r["step"] for r in rec[True]), 4)},
                step_pairs_bm64_faster=sum(b["step"] < a["step"] for a, b in zip(rec[False], rec[True])),
                conv3x3_ms={"bm128": round(med(sum(r["launches"]) for r in rec[False]), 4), "bm64": round(med(sum(r["launches"]) for r in rec[True]), 4)},
                conv3x3_pairs_bm64_faster=sum(sum(b["launches"]) < sum(a["launches"]) for a, b in zip(rec[False], rec[True])),
                launch_ms={"bm128": [round(med(r["launches"][j] for r in rec[False]), 4) for j in range(n_launch)],
                           "bm64": [round(med(r["launches"][j] for r in rec[True]), 4) for j in range(n_launch)]},
                launch_pairs_bm64_faster=[sum(b["launches"][j] < a["launches"][j] for a, b in zip(rec[False], rec[True])) for j in range(n_launch)],
                launch_order="invariant (I >= 2), G-Net per iteration, mask head")
    del model, inp
    torch.cuda.empty_cache()
    return line


def forward_wall(n_pairs, warmup, dev):
    """MAGNET.forward at one frame, stand-in backbones, host wall time per call (synchronised)."""
    from magnet_amd.standin import StubDNet, StubFNet, seeded_magnet_weights
    wl = synth.WORKLOADS["shipped"]
    m = MAGNET(bench.make_args(wl, wl.iters), d_net=StubDNet(1), f_net=StubFNet(2, fdim=wl.F), feat_dtype=wl.feat_dtype)
    seeded_magnet_weights(m, 3)
    m = m.to(dev).eval()
    inp = bench.device_inputs(wl, 1, seed=1000, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    ref = torch.rand(1, 3, 4 * wl.h, 4 * wl.w, generator=g, device=dev)
    nb = torch.rand(wl.V, 3, 4 * wl.h, 4 * wl.w, generator=g, device=dev)

    def call(mode):
        ConvStackMFMA.small_tiles = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            m(ref, nb, inp["nghbr_poses"], inp["is_valid"], inp["cam_intrins"], mode="test")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    try:
        for mode in (False, True):
            for _ in range(warmup):
                call(mode)
        rec = {False: [], True: []}
        for i in range(n_pairs):
            for mode in ((False, True) if i % 2 == 0 else (True, False)):
                rec[mode].append(call(mode))
    finally:
        ConvStackMFMA.small_tiles = "auto"
    return dict(kind="forward_wall", workload="shipped", frames=1, backbones="stand-in (StubDNet, StubFNet)", pairs=n_pairs,
                wall_ms={"bm128": round(statistics.median(rec[False]), 4), "bm64": round(statistics.median(rec[True]), 4)},
                pairs_bm64_faster=sum(b < a for a, b in zip(rec[False], rec[True])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="shipped,C2,C4")
    ap.add_argument("--frames", default="1,2,3,4,8")
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "latency", "bench_latency.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latency.py needs an MI355X")
    lib.load()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(line):
            line["device"] = torch.cuda.get_device_name(0)
            s = json.dumps(line)
            print(s, flush=True)
            f.write(s + "\n"); f.flush()
        for wl in a.workloads.split(","):
            for B in (int(x) for x in a.frames.split(",")):
                emit(measure(wl, B, a.pairs, a.warmup, dev))
        emit(forward_wall(a.pairs, a.warmup, dev))


if __name__ == "__main__":
    main()
