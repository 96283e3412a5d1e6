"""The D-Net's EfficientNet-B5 encoder, HIP against torch (magnet_amd/encoder.py): one process, one seeded module, the same images.  The
yardstick is torch's fp32 eval forward of the same module on the same GPU.  After --warmup calls of each, --pairs interleaved pairs are
timed with a host clock around work that ends in a device synchronise.  Then one more HIP call with EncoderMFMA.event_sink set gives
the per-layer times (HIP events around every launch, summed by layer kind and by stage), and the end-to-end times follow with the real
encoder in place of the stand-in: the stand-alone D-Net (DNET(dnet=True), both backends of encoder and decoder) and, with --magnet,
MAGNET.forward at the C2 workload.  Prints one JSON line per shape; --out FILE appends the lines.
--precision fp16 adds, per shape, a second line ("bench": "encoder_precision"): --pairs interleaved pairs of an fp16 runner against the
bf16x3 runner ON THE SAME MODULE (EncoderMFMA(model, precision="fp16"); the yardstick is the default path in the same process), the
fp16 side's events by launch kind and by stage next to the bf16x3 side's, the fp16 taps' differences from torch fp32, and the
stand-alone D-Net end to end with every fp16 mode on (encoder and decoder) against all off.

    python tools/bench_encoder.py [--pairs 12] [--warmup 3] [--shapes 1x480x640,5x480x640,3x352x1216] [--precision fp16]
                                  [--out profiles/encoder/bench_encoder.jsonl]
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


def clock(fn):
    """Host milliseconds of fn() up to the device having finished it."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pairs_of(a_fn, b_fn, warmup, pairs):
    """Interleaved timing of two callables: ([ms of a], [ms of b]); neither side always goes first."""
    for _ in range(warmup):
        a_fn(); b_fn()
    ta, tb = [], []
    for i in range(pairs):
        for k in ((0, 1) if i % 2 == 0 else (1, 0)):
            ms, _ = clock(a_fn if k == 0 else b_fn)
            (ta if k == 0 else tb).append(ms)
    return ta, tb


def layer_times(enc, img):
    """{kind: ms} and {stage: ms} of one warm HIP call, from the events around every launch."""
    from magnet_amd.encoder import EncoderMFMA
    EncoderMFMA.event_sink = sink = []
    try:
        enc(img)
        torch.cuda.synchronize()
    finally:
        EncoderMFMA.event_sink = None
    kinds, stages, total = {}, {}, 0.0
    for e0, e1, _flops, name in sink:
        ms = e0.elapsed_time(e1)
        kind = name.rsplit(".", 1)[-1] if name.startswith("blocks.") else name
        stage = name.split(".")[1] if name.startswith("blocks.") else name
        kinds[kind] = kinds.get(kind, 0.0) + ms
        stages[stage] = stages.get(stage, 0.0) + ms
        total += ms
    r = lambda d: {k: round(v, 4) for k, v in d.items()}
    return r(kinds), r(stages), round(total, 4), len(sink)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="1x480x640,5x480x640,3x352x1216")
    ap.add_argument("--magnet", action="store_true", help="also time MAGNET.forward (C2 workload) with the real encoder on both backends")
    ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "fp16"],
                    help="fp16: also pair the fp16 runner against the bf16x3 runner on the same module, with its own per-kind and per-stage events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from magnet_amd import lib
    from magnet_amd.dnet import DNET, load_seeded_decoder
    from magnet_amd.encoder import Encoder, EncoderMFMA, load_seeded_encoder
    from magnet_amd.standin import make_dnet_args
    lib.load()
    dev = torch.device("cuda:0")
    hip = load_seeded_encoder(Encoder(backend="hip"), 0).to(dev).eval()
    ref = Encoder().to(dev).eval()
    ref.load_state_dict(hip.state_dict())
    dn = {}
    for eb, db in (("torch", "torch"), ("torch", "hip"), ("hip", "hip")):
        d = DNET(make_dnet_args(), Encoder(backend=eb), dnet=True, backend=db)
        d.d_net.encoder.load_state_dict(hip.state_dict())
        load_seeded_decoder(d.d_net.decoder, 0)
        dn[(eb, db)] = d.to(dev).eval()
    f16 = dn16 = None
    if a.precision == "fp16":
        f16 = EncoderMFMA(hip.original_model, precision="fp16")      # a second runner on the SAME module
        dn16 = DNET(make_dnet_args(), Encoder(backend="hip", precision="fp16"), dnet=True, backend="hip", precision="fp16")
        dn16.load_state_dict(dn[("hip", "hip")].state_dict())
        dn16 = dn16.to(dev).eval()
    med = statistics.median

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")

    for shape in a.shapes.split(","):
        N, H, W = (int(v) for v in shape.split("x"))
        img = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
        with torch.no_grad():
            t_hip, t_ref = pairs_of(lambda: hip(img), lambda: ref(img), a.warmup, a.pairs)
            kinds, stages, ev_total, launches = layer_times(hip, img)
            got, want = hip(img), ref(img)
            diff = {str(i): float((got[i] - want[i]).abs().max() / want[i].abs().max()) for i in (4, 5, 6, 8, 11)}
            line = {"bench": "encoder", "shape": [N, H, W], "pairs": a.pairs, "gpu": torch.cuda.get_device_name(0),
                    "hip_ms": [round(v, 3) for v in t_hip], "torch_ms": [round(v, 3) for v in t_ref],
                    "hip_ms_median": round(med(t_hip), 3), "torch_ms_median": round(med(t_ref), 3),
                    "pairs_won": {"hip": sum(x < y for x, y in zip(t_hip, t_ref)), "torch": sum(y < x for x, y in zip(t_hip, t_ref))},
                    "launches": launches, "event_ms_total": ev_total, "ms_by_kind": kinds, "ms_by_stage": stages,
                    "max_rel_diff_hip_vs_torch": diff}
            del got, want
            t_a, t_b = pairs_of(lambda: dn[("hip", "hip")](img), lambda: dn[("torch", "hip")](img), a.warmup, a.pairs)
            t_c, _ = pairs_of(lambda: dn[("torch", "torch")](img), lambda: None, 1, max(3, a.pairs // 4))
            line["dnet_ms_median"] = {"encoder hip + decoder hip": round(med(t_a), 3), "encoder torch + decoder hip": round(med(t_b), 3),
                                      "encoder torch + decoder torch": round(med(t_c), 3)}
        emit(line)
        if f16 is not None:
            with torch.no_grad():
                t_f, t_b = pairs_of(lambda: f16(img), lambda: hip(img), a.warmup, a.pairs)
                k16, s16, ev16, n16 = layer_times(f16, img)
                got, want = f16(img), ref(img)
                diff16 = {str(i): float((got[i] - want[i]).abs().max() / want[i].abs().max()) for i in (4, 5, 6, 8, 11)}
                del got, want
                t_d16, t_d = pairs_of(lambda: dn16(img), lambda: dn[("hip", "hip")](img), a.warmup, a.pairs)
            emit({"bench": "encoder_precision", "shape": [N, H, W], "pairs": a.pairs, "gpu": torch.cuda.get_device_name(0),
                  "fp16_ms": [round(v, 3) for v in t_f], "bf16x3_ms": [round(v, 3) for v in t_b],
                  "fp16_ms_median": round(med(t_f), 3), "bf16x3_ms_median": round(med(t_b), 3),
                  "pairs_won": {"fp16": sum(x < y for x, y in zip(t_f, t_b)), "bf16x3": sum(y < x for x, y in zip(t_f, t_b))},
                  "launches": {"fp16": n16, "bf16x3": launches}, "event_ms_total": {"fp16": ev16, "bf16x3": ev_total},
                  "ms_by_kind": {"fp16": k16, "bf16x3": kinds}, "ms_by_stage": {"fp16": s16, "bf16x3": stages},
                  "max_rel_diff_fp16_vs_torch": diff16,
                  "dnet_ms": {"all fp16": [round(v, 3) for v in t_d16], "all bf16x3": [round(v, 3) for v in t_d]},
                  "dnet_ms_median": {"all fp16": round(med(t_d16), 3), "all bf16x3": round(med(t_d), 3)},
                  "dnet_pairs_won": {"all fp16": sum(x < y for x, y in zip(t_d16, t_d)), "all bf16x3": sum(y < x for x, y in zip(t_d16, t_d))}})
            f16._bufs.clear(); f16._bufs_sig = None
        for d in list(dn.values()) + ([dn16] if dn16 is not None else []):     # one shape's buffers at a time
            if d._runner is not None:
                d._runner._bufs.clear(); d._runner._bufs_sig = None
            r = getattr(d.d_net.encoder, "_runner", None)
            if r is not None:
                r._bufs.clear(); r._bufs_sig = None
        hip._runner._bufs.clear(); hip._runner._bufs_sig = None
        torch.cuda.empty_cache()
    if a.magnet:
        magnet_forward(a, dev, hip.state_dict())


def magnet_forward(a, dev, enc_state):
    """MAGNET.forward at C2 (B = 1, V = 4, 480 x 640) with the real encoder inside the D-Net: HIP against torch encoder, same decoder path."""
    from magnet_amd import fnet, synth
    from magnet_amd.dnet import DNET, load_seeded_decoder
    from magnet_amd.encoder import Encoder
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import make_args, make_dnet_args, seeded_magnet_weights
    wl = synth.WORKLOADS["C2"]
    V = 4
    models = {}
    for eb in ("hip", "torch"):
        args = make_args(D=wl.D, iters=wl.iters, dpv_h=wl.h, dpv_w=wl.w, fdim=64, V=V)
        args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
        d = DNET(make_dnet_args(), Encoder(backend=eb), backend="hip")
        d.d_net.encoder.load_state_dict(enc_state)
        load_seeded_decoder(d.d_net.decoder, 0)
        with torch.no_grad():                                       # standin.make_dnet's depth prior: plausible scenes for the matcher
            d.d_net.decoder.depth_head[4].weight.mul_(0.25)
            d.d_net.decoder.depth_head[4].bias.copy_(torch.tensor([2.5, -3.0]))
        m = MAGNET(args, d_net=d, f_net=fnet.FNET(args), feat_dtype=wl.feat_dtype, dnet_backend="hip").to(dev).eval()
        seeded_magnet_weights(m, seed=4)
        models[eb] = m
    models["torch"].load_state_dict(models["hip"].state_dict())
    g = torch.Generator().manual_seed(2)
    ref_img = torch.rand(1, 3, 4 * wl.h, 4 * wl.w, generator=g).to(dev)
    src_img = torch.rand(V, 3, 4 * wl.h, 4 * wl.w, generator=g).to(dev)
    poses = synth.make_poses(wl.camera, 1, V, g).to(dev)
    intr = synth.make_intrinsics(wl.camera, wl.h, wl.w, 1)
    valid = torch.ones(1, V, dtype=torch.int32)
    run = lambda m: (lambda: m(ref_img, src_img, poses, valid, intr, mode="test"))
    with torch.no_grad():
        t_h, t_t = pairs_of(run(models["hip"]), run(models["torch"]), a.warmup, a.pairs)
    line = {"bench": "magnet_forward", "config": "C2", "V": V, "pairs": a.pairs, "encoder_hip_ms_median": round(statistics.median(t_h), 3),
            "encoder_torch_ms_median": round(statistics.median(t_t), 3), "encoder_hip_ms": [round(v, 3) for v in t_h],
            "encoder_torch_ms": [round(v, 3) for v in t_t]}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
