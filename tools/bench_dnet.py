"""Timing of the D-Net decoder (DenseDepth_BN at downsample ratio 4, magnet_amd/dnet.py) on one GPU: the torch module in fp32 eval
mode (MIOpen; its output passed through activation_G_magnet) against DNetMFMA (matrix-core path, writing the reference frames' x_d3
into a G-Net input buffer in place), on the stand-in encoder's features (the encoder is not timed):
  * C2 (480 x 640, V = 4) with B = 1 and B = 4 frames (5 and 20 images), KITTI (352 x 1216, V = 2, B = 1: 3 images);
  * MAGNET.forward at C2, B = 1, D = 64, I = 3 with the stand-in encoder and a PSMNet F-Net (matrix-core), dnet_backend 'torch' / 'hip'.
Also the HIP decoder's time per convolution layer class (CUDA events around each launch) at C2, B = 1.  Prints one JSON line per
measurement; --out FILE appends them.

--standalone times the stand-alone D-Net instead (DNET(dnet=True): decoder + depth head + mask head + learned convex upsampling +
activation_G, encoder not timed): torch fp32 against DNetMFMA.run_standalone at C2 with N = 1 (the way test_DNet.py feeds it) and
N = 4 and at KITTI with N = 1, plus the per-launch event times and the time of everything behind x_feat (the two head launches and
magnet_dnet_upsample_gauss).  Each timing is the median of --repeats timed loops of --steps calls.

--split_k sweep times every plain decoder launch (event-bracketed, the reduce launch included) with the split-K factor S forced to 1, 2, 3,
4, 5, 6 and 8 on all layers (a layer whose input has too few chunks for S keeps its largest allowed factor) at 480 x 640 with N = 1, 2, 4
and 352 x 1216 with N = 1, 3, and prints what dnet.split_factor would choose.  --split_k auto --pairs P times P interleaved pairs, in this
process, of DNetMFMA(split_k=0) against DNetMFMA(split_k="auto") for run_standalone and run at N = 1 (both shapes) and N = 4, checks that
split_k=0 gives the default runner's bits and reports how far "auto" is from them.

--precision fp16 --pairs P times P interleaved pairs, in this process, of DNetMFMA(precision="bf16x3") against DNetMFMA(precision="fp16")
for run and run_standalone, each with split_k 0 and "auto", at 480 x 640 with N = 1, 5, 20 and 352 x 1216 with N = 1, 3, with the
per-launch event times of both; then x_feat / mu / sigma of both modes against a float64 decoder at C2 (N = 5) and KITTI (N = 3), the
peak activation and folded-weight magnitudes (the headroom to 65504), and MAGNET.forward's final depth at C2 / I = 3 under
dnet_precision 'fp16' against the default mode and against the torch decoder, per refinement.  Every line carries the SHA-256 of the
default mode's outputs, so two builds can be compared on the default path.

    python tools/bench_dnet.py [--steps 10] [--warmup 3] [--out profiles/dnet/bench_dnet.jsonl]
    python tools/bench_dnet.py --split_k sweep [--repeats 7] [--out profiles/splitk/bench_splitk.jsonl]
    python tools/bench_dnet.py --split_k auto --pairs 12 [--steps 20] [--out profiles/splitk/bench_splitk.jsonl]
    python tools/bench_dnet.py --precision fp16 --pairs 12 [--steps 20] [--out profiles/dnet_precision/bench_dnet_precision.jsonl]
    python tools/bench_dnet.py --standalone [--steps 20] [--warmup 5] [--repeats 5] [--out profiles/dnet/bench_dnet_standalone.jsonl]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-magnet", action="store_true")
    ap.add_argument("--standalone", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--split_k", default=None, choices=["sweep", "auto"])
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--precision", default=None, choices=["fp16"])
    a = ap.parse_args()
    from magnet_amd import fnet, lib, synth
    from magnet_amd.dnet import DNetMFMA, gaussian_activation
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import make_args, make_dnet, seeded_magnet_weights
    lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        d["gpu"] = torch.cuda.get_device_name(0)
        lines.append(d)
        print(json.dumps(d), flush=True)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / a.steps, 3)

    def images(n, H, W, seed):
        return torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)

    def write_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                for d_ in lines:
                    fh.write(json.dumps(d_) + "\n")

    if a.precision:
        import copy
        import hashlib
        import statistics
        from magnet_amd.planes import fold_bn
        d = make_dnet(dnet=True).to(dev)
        dec = d.d_net.decoder

        def sha(*ts):
            h = hashlib.sha256()
            for t in ts:
                h.update(t.detach().contiguous().cpu().numpy().tobytes())
            return h.hexdigest()[:16]

        def once(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.steps

        def launches_ms(runner, feats):
            """median event time of every bracketed launch of run_standalone, keyed by launch_log's layer names (+ the tail kernel)"""
            per = []
            for _ in range(a.repeats + 2):
                sink = []
                DNetMFMA.event_sink = sink
                runner.run_standalone(feats)
                torch.cuda.synchronize()
                DNetMFMA.event_sink = None
                per.append([e0.elapsed_time(e1) for e0, e1, _ in sink])
            names = [l for l, _ in runner.launch_log] + ["upsample_gauss"]
            return {n: round(statistics.median(col), 4) for n, col in zip(names, zip(*per[2:]))}

        for name, H, W, N in (("C2", 480, 640, 1), ("C2", 480, 640, 5), ("C2", 480, 640, 20), ("KITTI", 352, 1216, 1), ("KITTI", 352, 1216, 3)):
            with torch.no_grad():
                feats = d.d_net.encoder(images(N, H, W, N))
                for sk in (0, "auto"):
                    r3, r16 = DNetMFMA(dec, split_k=sk), DNetMFMA(dec, split_k=sk, precision="fp16")
                    o3, o16 = r3.run_standalone(feats), r16.run_standalone(feats)
                    g3, f3 = r3.run(feats)
                    used = {n: S for n, _, S in r16.factors_used}
                    for form, f_3, f_16 in (("run_standalone", lambda: r3.run_standalone(feats), lambda: r16.run_standalone(feats)),
                                            ("run", lambda: r3.run(feats), lambda: r16.run(feats))):
                        for _ in range(a.warmup):
                            f_3(); f_16()
                        t3, t16 = [], []
                        for _ in range(a.pairs):
                            t3.append(once(f_3)); t16.append(once(f_16))
                        emit(dict(bench="dnet_precision_pairs", shape=name, H=H, W=W, N=N, form=form, split_k=sk, pairs=a.pairs, steps=a.steps,
                                  factors=used, ms_bf16x3=[round(t, 4) for t in t3], ms_fp16=[round(t, 4) for t in t16],
                                  median_bf16x3=round(statistics.median(t3), 4), median_fp16=round(statistics.median(t16), 4),
                                  fp16_faster_pairs=sum(b < a_ for a_, b in zip(t3, t16)),
                                  sha_default_standalone=sha(o3), sha_default_run=sha(g3, f3),
                                  standalone_rel_diff_to_default=float((o16.double() - o3.double()).abs().max() / o3.double().abs().max())))
                    emit(dict(bench="dnet_precision_layers", shape=name, H=H, W=W, N=N, split_k=sk, factors=used,
                              ms_bf16x3=launches_ms(r3, feats), ms_fp16=launches_ms(r16, feats)))
                    del r3, r16, o3, o16, g3, f3
            del feats
            torch.cuda.empty_cache()

        # accuracy against a float64 decoder, seeded weights; headroom to 65504
        rel = lambda x, y: float((x.double() - y.double()).abs().max() / y.double().abs().max())
        dm = make_dnet().to(dev)
        decm = dm.d_net.decoder
        for name, H, W, N in (("C2", 480, 640, 5), ("KITTI", 352, 1216, 3)):
            with torch.no_grad():
                feats = dm.d_net.encoder(images(N, H, W, N))
                dec64 = copy.deepcopy(decm).double().eval()
                ref_g, ref_f = gaussian_activation(dec64([None if f is None else f.double() for f in feats]))
                del dec64
                out = {}
                for prec in ("bf16x3", "fp16"):
                    r = DNetMFMA(decm, precision=prec)
                    g, f = r(feats)
                    out[prec] = dict(x_feat=rel(f, ref_f), mu=rel(g[:, 0], ref_g[:, 0]), sigma=rel(g[:, 1], ref_g[:, 1]))
                    if prec == "fp16":
                        b = r._bufs
                        peaks = {k: float(v.float().abs().max()) for k, v in b.items() if isinstance(v, torch.Tensor) and k != "splitk.work"}
                emit(dict(bench="dnet_precision_accuracy", shape=name, H=H, W=W, N=N, rel_to_fp64=out, peak_activation=peaks,
                          peak_encoder_feature=max(float(feats[i].abs().max()) for i in (5, 6, 8, 11))))
            del feats, ref_g, ref_f
            torch.cuda.empty_cache()
        wmax = {"conv2": float(decm.conv2.weight.abs().max())}
        for up in ("up1", "up2", "up3"):
            net = getattr(decm, up)._net
            wmax[up + ".0"] = float(fold_bn(net[0], net[1])[0].abs().max())
            wmax[up + ".1"] = float(fold_bn(net[3], net[4])[0].abs().max())
        emit(dict(bench="dnet_precision_weights", peak_folded_weight=wmax, limit=65504.0))

        # MAGNET.forward at C2 / I = 3: final depth per refinement, fp16 decoder against the default HIP decoder and the torch decoder
        args = make_args(D=64, iters=3, dpv_h=120, dpv_w=160, fdim=64, V=4)
        args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
        torch.manual_seed(0)
        f = fnet.FNET(args)
        wl = synth.Workload("C2", "scannet", 120, 160, V=4, D=64, iters=3)
        inp = synth.make_inputs(wl, B=1, seed=5)
        ref_img, nb = images(1, 480, 640, 1), images(4, 480, 640, 2)
        poses = inp["nghbr_poses"].to(dev)
        preds, ms = {}, {}
        for key, kw in (("torch", dict(dnet_backend="torch")), ("hip", dict(dnet_backend="hip")),
                        ("hip_fp16", dict(dnet_backend="hip", dnet_precision="fp16"))):
            model = MAGNET(args, d_net=dm, f_net=f, **kw).to(dev).eval()
            seeded_magnet_weights(model, seed=4)
            with torch.no_grad():
                preds[key] = [p.clone() for p in model(ref_img, nb, poses, inp["is_valid"], inp["cam_intrins"], mode="test")]
                ms[key] = timed(lambda: model(ref_img, nb, poses, inp["is_valid"], inp["cam_intrins"], mode="test"))
            del model
            torch.cuda.empty_cache()
        abs_rel = lambda x, y: [float(((g[:, 0] - r[:, 0]).abs() / r[:, 0].abs()).mean()) for g, r in zip(x, y)]
        emit(dict(bench="dnet_precision_magnet", shape="C2", B=1, V=4, D=64, iters=3, ms_forward=ms,
                  abs_rel_fp16_vs_default_hip=abs_rel(preds["hip_fp16"], preds["hip"]),
                  abs_rel_fp16_vs_torch=abs_rel(preds["hip_fp16"], preds["torch"]),
                  abs_rel_default_hip_vs_torch=abs_rel(preds["hip"], preds["torch"]), sha_default_hip=sha(*preds["hip"])))
        write_out()
        return

    if a.split_k:
        import statistics
        from magnet_amd.dnet import SPLIT_LAYERS, split_factor
        d = make_dnet(dnet=True).to(dev)
        dec = d.d_net.decoder
        chunks = dict(zip(SPLIT_LAYERS, (64, 70, 32, 34, 16, 18, 8)))
        n_tiles = dict(zip(SPLIT_LAYERS, (16, 8, 8, 4, 4, 2, 2)))

        def layer_ms(runner, feats, reps):
            """median event time per plain decoder launch of run_standalone (the first len(SPLIT_LAYERS) brackets), and the rows of each"""
            per = []
            for _ in range(reps + 2):
                sink = []
                DNetMFMA.event_sink = sink
                runner.run_standalone(feats)
                torch.cuda.synchronize()
                DNetMFMA.event_sink = None
                per.append([e0.elapsed_time(e1) for e0, e1, _ in sink])
            ms = [round(statistics.median(col), 4) for col in zip(*per[2:])]
            return dict(zip(SPLIT_LAYERS, ms)), round(sum(ms[:len(SPLIT_LAYERS)]), 4), {n: r for n, r, _ in runner.factors_used}

        if a.split_k == "sweep":
            for name, H, W, N in (("C2", 480, 640, 1), ("C2", 480, 640, 2), ("C2", 480, 640, 4), ("KITTI", 352, 1216, 1), ("KITTI", 352, 1216, 3)):
                with torch.no_grad():
                    feats = d.d_net.encoder(images(N, H, W, N))
                    for S in (1, 2, 3, 4, 5, 6, 8):
                        forced = {n: min(S, max(1, chunks[n] // lib.SPLITK_MIN_CHUNKS)) for n in SPLIT_LAYERS}
                        ms, total, rows = layer_ms(DNetMFMA(dec, split_k=forced), feats, a.repeats)
                        emit(dict(bench="dnet_splitk_sweep", shape=name, H=H, W=W, N=N, S=S, forced=forced, ms_per_layer=ms,
                                  ms_all_launches=total, repeats=a.repeats,
                                  workgroups={n: (rows[n] + 127) // 128 * n_tiles[n] for n in SPLIT_LAYERS},
                                  auto={n: split_factor((rows[n] + 127) // 128, n_tiles[n], chunks[n]) for n in SPLIT_LAYERS}))
                del feats
                torch.cuda.empty_cache()
            write_out()
            return

        def once(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.steps

        for name, H, W, N in (("C2", 480, 640, 1), ("KITTI", 352, 1216, 1), ("C2", 480, 640, 4)):
            with torch.no_grad():
                feats = d.d_net.encoder(images(N, H, W, N))
                r_def, r0, r1 = DNetMFMA(dec), DNetMFMA(dec, split_k=0), DNetMFMA(dec, split_k="auto")
                base, o0, o1 = r_def.run_standalone(feats), r0.run_standalone(feats), r1.run_standalone(feats)
                used = {n: S for n, _, S in r1.factors_used}
                rel = float((o1.double() - base.double()).abs().max() / base.double().abs().max())
                for form, f0, f1 in (("run_standalone", lambda: r0.run_standalone(feats), lambda: r1.run_standalone(feats)),
                                     ("run", lambda: r0.run(feats), lambda: r1.run(feats))):
                    for _ in range(a.warmup):
                        f0(); f1()
                    t0s, t1s = [], []
                    for _ in range(a.pairs):
                        t0s.append(once(f0)); t1s.append(once(f1))
                    emit(dict(bench="dnet_splitk_pairs", shape=name, H=H, W=W, N=N, form=form, pairs=a.pairs, steps=a.steps,
                              factors=used, ms_split0=[round(t, 4) for t in t0s], ms_auto=[round(t, 4) for t in t1s],
                              median_split0=round(statistics.median(t0s), 4), median_auto=round(statistics.median(t1s), 4),
                              auto_faster_pairs=sum(b < a_ for a_, b in zip(t0s, t1s)),
                              split0_bits_equal_default=bool(torch.equal(base, o0)), auto_rel_diff_to_default=rel))
                ms0, tot0, _ = layer_ms(r0, feats, a.repeats)
                ms1, tot1, _ = layer_ms(r1, feats, a.repeats)
                emit(dict(bench="dnet_splitk_layers", shape=name, H=H, W=W, N=N, factors=used, ms_split0=ms0, ms_auto=ms1,
                          ms_split0_launches=tot0, ms_auto_launches=tot1))
            del feats
            torch.cuda.empty_cache()
        write_out()
        return

    if a.standalone:
        import statistics
        d = make_dnet(dnet=True).to(dev)
        dec = d.d_net.decoder
        runner = DNetMFMA(dec)

        def median_ms(fn):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            reps = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                reps.append((time.perf_counter() - t0) * 1e3 / a.steps)
            return round(statistics.median(reps), 3), round(min(reps), 3), round(max(reps), 3)

        for name, H, W, N in (("C2", 480, 640, 1), ("C2", 480, 640, 4), ("KITTI", 352, 1216, 1)):
            with torch.no_grad():
                feats = d.d_net.encoder(images(N, H, W, N))
                # interleaved A/B/A/B: both forms see the same clocks
                t_torch = median_ms(lambda: gaussian_activation(dec(feats), magnet=False))
                t_hip = median_ms(lambda: runner.run_standalone(feats))
                t_torch2 = median_ms(lambda: gaussian_activation(dec(feats), magnet=False))
                t_hip2 = median_ms(lambda: runner.run_standalone(feats))
                per = []
                for _ in range(5):
                    sink = []
                    DNetMFMA.event_sink = sink
                    runner.run_standalone(feats)
                    torch.cuda.synchronize()
                    DNetMFMA.event_sink = None
                    per.append([e0.elapsed_time(e1) for e0, e1, _ in sink])
            ms = [round(statistics.median(col), 3) for col in zip(*per)]
            mt, mh = min(t_torch[0], t_torch2[0]), max(t_hip[0], t_hip2[0])      # the comparison least favourable to the HIP form
            emit(dict(bench="dnet_standalone", shape=name, H=H, W=W, N=N, steps=a.steps, warmup=a.warmup, repeats=a.repeats,
                      ms_torch_fp32=[t_torch, t_torch2], ms_hip=[t_hip, t_hip2], speedup_worst_case=round(mt / mh, 2),
                      hip_faster=bool(mh < mt), launches=len(ms), ms_per_launch=ms, ms_decoder_convs=round(sum(ms[:-3]), 3),
                      ms_depth_head=ms[-3], ms_mask_head=ms[-2], ms_upsample_gauss=ms[-1], ms_behind_x_feat=round(sum(ms[-3:]), 3)))
            del feats
            torch.cuda.empty_cache()
        write_out()
        return

    d = make_dnet().to(dev)
    dec = d.d_net.decoder
    runner = DNetMFMA(dec)
    for name, H, W, B, V in (("C2", 480, 640, 1, 4), ("C2", 480, 640, 4, 4), ("KITTI", 352, 1216, 1, 2)):
        N = B * (1 + V)
        with torch.no_grad():
            feats = d.d_net.encoder(images(N, H, W, N))
            h, w = feats[5].shape[2:]
            ctot, c_off = 320, 64
            ghi = torch.zeros((B * (h + 2) * (w + 2), ctot), dtype=torch.bfloat16, device=dev); glo = torch.zeros_like(ghi)
            t_torch = timed(lambda: gaussian_activation(dec(feats)))
            t_hip = timed(lambda: runner.run(feats, n_ref=B, x_d3_out=(ghi, glo, ctot, c_off)))
            t_hip_nchw = timed(lambda: runner(feats))
        emit(dict(bench="dnet_decoder", shape=name, H=H, W=W, B=B, V=V, images=N, steps=a.steps, warmup=a.warmup,
                  ms_torch_fp32=t_torch, ms_hip_in_place=t_hip, ms_hip_nchw=t_hip_nchw, speedup=round(t_torch / t_hip, 2)))
        if name == "C2" and B == 1:
            sink = []
            DNetMFMA.event_sink = sink
            with torch.no_grad():
                runner.run(feats, n_ref=B, x_d3_out=(ghi, glo, ctot, c_off))
            torch.cuda.synchronize()
            DNetMFMA.event_sink = None
            ms = [e0.elapsed_time(e1) for e0, e1, _ in sink]
            fl = [f for _, _, f in sink]
            emit(dict(bench="dnet_decoder_layers", shape=name, B=B, launches=len(sink),
                      ms_per_launch=[round(x, 3) for x in ms], tflops_per_launch=[round(f / (x * 1e9), 1) for f, x in zip(fl, ms)],
                      ms_conv_total=round(sum(ms), 3), gflop_total=round(sum(fl) / 1e9, 1)))
        del feats, ghi, glo
        torch.cuda.empty_cache()

    if not a.skip_magnet:
        args = make_args(D=64, iters=3, dpv_h=120, dpv_w=160, fdim=64, V=4)
        args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
        torch.manual_seed(0)
        f = fnet.FNET(args)
        wl = synth.Workload("C2", "scannet", 120, 160, V=4, D=64, iters=3)
        inp = synth.make_inputs(wl, B=1, seed=5)
        ref_img, nb = images(1, 480, 640, 1), images(4, 480, 640, 2)
        poses = inp["nghbr_poses"].to(dev)
        res = {}
        for be in ("torch", "hip"):
            model = MAGNET(args, d_net=d, f_net=f, dnet_backend=be).to(dev).eval()
            seeded_magnet_weights(model, seed=4)
            with torch.no_grad():
                res[be] = timed(lambda: model(ref_img, nb, poses, inp["is_valid"], inp["cam_intrins"], mode="test"))
            del model
            torch.cuda.empty_cache()
        emit(dict(bench="magnet_forward", shape="C2", B=1, V=4, D=64, iters=3, encoder="standin", fnet="PSMNet (matrix-core)",
                  steps=a.steps, warmup=a.warmup, ms_dnet_torch=res["torch"], ms_dnet_hip=res["hip"],
                  speedup=round(res["torch"] / res["hip"], 2)))
    write_out()


if __name__ == "__main__":
    main()
