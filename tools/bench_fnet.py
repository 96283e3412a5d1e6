"""Time the F-Net (row N3) on one GPU at the reference's inference shape (480x640 ScanNet images, 5 images per
reference frame): matrix-core path (FNetMFMA, output in the matcher's layouts) vs the same torch module on MIOpen
(fp32, NCHW) + the pack pass it needs.  One JSON line.  --profile-layers prints per-layer time / TFLOP/s.
--precision {bf16x3,fp16} selects the runner's precision; --pairs N runs an interleaved A/B of the two precisions on this box (one
JSON line per pair, fp16 and bf16x3 timed back to back in alternating order, then a summary line; with --profile-layers the per-layer
table of both)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magnet_amd import fnet, lib  # noqa: E402


def conv_flops(psm, H, W):
    """Multiply-add flops (x2) of every convolution of one image."""
    tot = 0.0
    x = torch.zeros(1, 3, H, W)
    hooks = []

    def hook(m, i, o):
        nonlocal tot
        tot += 2.0 * o.numel() * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
    for m in psm.modules():
        if isinstance(m, torch.nn.Conv2d):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        psm(x)
    for h in hooks:
        h.remove()
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8, help="reference frames per step (x5 images)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--feat-dtype", default="bf16")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--profile-layers", action="store_true")
    ap.add_argument("--no-split", action="store_true", help="one stream for the whole batch (default: two half-batches on two streams)")
    ap.add_argument("--parts", type=int, default=0, help="dev: number of part-batches / streams (0 = the runner's default)")
    ap.add_argument("--dev-lib", action="store_true", help="bind to libmagnet_hip_dev.so (MAGNET_CONV_VARIANT A/B)")
    ap.add_argument("--precision", choices=fnet.FNetMFMA.PRECISIONS, default="bf16x3", help="FNetMFMA(psm, precision=...)")
    ap.add_argument("--pairs", type=int, default=0, help="interleaved A/B: N pairs of (fp16, bf16x3) timings; ignores --precision")
    a = ap.parse_args()
    if a.dev_lib:
        lib.use_dev_build()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    psm = fnet.PSMNet(feature_dim=64).eval()
    flops_img = conv_flops(psm, a.height, a.width)
    psm = psm.to(dev)
    N = 5 * a.frames
    img = torch.randn(N, 3, a.height, a.width, device=dev)
    def runner(precision):
        r = fnet.FNetMFMA(psm, precision=precision)
        if a.parts:
            r.split_parts = a.parts
        if a.no_split:
            r.split_min_images = 10 ** 9
        return r

    run = runner(a.precision)
    if a.profile_layers and not a.pairs:                   # (per-layer events of two overlapping chains would not add up to the wall time)
        run.split_min_images = 10 ** 9

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps

    def layers(r, dt):
        """One pass on one stream with an event pair around every convolution launch."""
        keep, r.split_min_images = r.split_min_images, 10 ** 9
        names, conv = [], r._conv

        def named(name, *x, **k):                            # the sink's entries are in launch order: note the layer of each
            names.append(name)
            return conv(name, *x, **k)
        r._conv = named
        sink = fnet.FNetMFMA.event_sink = []
        try:
            r.run(img, n_ref=a.frames, feat_dtype=a.feat_dtype)
            torch.cuda.synchronize()
        finally:
            fnet.FNetMFMA.event_sink = None
            r.split_min_images = keep
            del r._conv
        tot = 0.0
        for i, (e0, e1, fl) in enumerate(sink):
            ms = e0.elapsed_time(e1); tot += ms
            print(f"  conv {i:3d}  {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TFLOP/s fp32-equiv  {names[i] if i < len(names) else ''}")
        print(f"  [{r.precision}] conv launches total {tot:.2f} ms (one stream){'' if dt is None else f' of {dt * 1e3:.2f} ms'}")

    if a.pairs:
        runs = {p: runner(p) for p in ("fp16", "bf16x3")}
        ms = {p: [] for p in runs}
        for i in range(a.pairs):
            order = ("fp16", "bf16x3") if i % 2 == 0 else ("bf16x3", "fp16")
            for p in order:
                ms[p].append(timed(lambda: runs[p].run(img, n_ref=a.frames, feat_dtype=a.feat_dtype)) * 1e3)
            print(json.dumps({"pair": i, "order": list(order), "ms_fp16": ms["fp16"][-1], "ms_bf16x3": ms["bf16x3"][-1]}))
        wins = sum(x < y for x, y in zip(ms["fp16"], ms["bf16x3"]))
        med = {p: sorted(v)[len(v) // 2] for p, v in ms.items()}
        print(json.dumps({"workload": f"F-Net PSMNet {a.height}x{a.width}, {N} images, interleaved A/B", "pairs": a.pairs, "fp16_wins": wins,
                          "ms_fp16_median": med["fp16"], "ms_bf16x3_median": med["bf16x3"], "ms_fp16_min": min(ms["fp16"]),
                          "ms_fp16_max": max(ms["fp16"]), "ms_bf16x3_min": min(ms["bf16x3"]), "ms_bf16x3_max": max(ms["bf16x3"]),
                          "images_per_s_fp16": N / med["fp16"] * 1e3, "images_per_s_bf16x3": N / med["bf16x3"] * 1e3,
                          "out": f"matcher layouts, {a.feat_dtype}", "streams": 1 if a.no_split else runs["fp16"].split_parts}))
        if a.profile_layers:
            for p in ("bf16x3", "fp16"):
                layers(runs[p], None)
        return

    dt = timed(lambda: run.run(img, n_ref=a.frames, feat_dtype=a.feat_dtype))
    rec = {"workload": f"F-Net PSMNet {a.height}x{a.width}, {N} images ({a.frames} ref frames x 5)", "ms_mfma": dt * 1e3,
           "images_per_s_mfma": N / dt, "gflop_per_image": flops_img / 1e9, "tflops_fp32_equiv_mfma": flops_img * N / dt / 1e12,
           "out": f"matcher layouts, {a.feat_dtype}", "streams": 1 if run.split_min_images > N else run.split_parts, "precision": a.precision}
    if not a.skip_torch:
        fe = lib.feat_enum(a.feat_dtype)

        def torch_path():
            with torch.no_grad():
                f = psm(img)
            lib.pack_features(f[:a.frames].contiguous(), fe, pad=0); lib.pack_features(f[a.frames:].contiguous(), fe, pad=1)
        dtt = timed(torch_path)
        rec.update({"ms_torch_miopen_fp32": dtt * 1e3, "images_per_s_torch": N / dtt, "speedup": dtt / dt})
    print(json.dumps(rec))
    if a.profile_layers:
        layers(run, dt)


if __name__ == "__main__":
    main()
