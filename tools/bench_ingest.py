"""Image ingest, host path against device path (magnet_amd/ingest.py, magnet_image_prep_u8).  One process on one MI355X.  Both sides
start from decoded frames (PIL RGB images of seeded random pixels: decoding is the same work on both sides and is left out) and end with
the (N, 3, H, W) fp32 tensor on the device, the device idle.

  (a) per shape, --pairs interleaved pairs, host clock around work that ends in a device synchronise, the side that goes first
      alternating:
        host    data.ScanNetFolder's lines: Pillow BILINEAR resize (KITTI: im.crop), numpy fp32 / 255, torch (x - mean) / std, stack,
                .to(device) of the fp32 tensor
        device  the raw_images=True lines: np.array(rgb) into a uint8 tensor, stack, ImagePrep.prep (uint8 upload + one launch)
      ms per frame of both, pairs won, and the outputs compared (differing elements: 0).
  (b) the kernel alone on frames already on the device (HIP events around --launches launches, per pair) against a device-to-device
      copy that moves the same total bytes (the crop box's bytes in + the fp32 output's bytes out = bytes read + written by the copy).
      Both sides walk a ring of buffer sets of --ring_mb in all (default 640 MB, beyond the 256 MB last-level cache), so no launch
      finds its input or output resident from the launch before: the rates are memory rates, not cache rates.  A walk once round the
      ring is replayed as a HIP graph (no host time between launches: kernel_us / copy_us); the eager launch-to-launch times, which
      include the host's time per call, are reported beside them (eager_*).
  (c) SequenceRunner at one new frame per step (C2: B = 1, V = 4, D = 64, 480x640; the matrix-core F-Net and the HIP decoder in the
      step), eager and graph=True: a runner fed host-normalised frames (host path, then add + refine) against a runner with
      image_prep fed the uint8 frame (add + refine), two runners over one model.

    python tools/bench_ingest.py [--pairs 12] [--warmup 3] [--parts a,b,c] [--out profiles/ingest/bench_ingest.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = (("scannet_1", 1, (968, 1296), (480, 640), False), ("scannet_5", 5, (968, 1296), (480, 640), False),
          ("kitti_1", 1, (375, 1242), (352, 1216), True))
OFFSETS = (-2, -1, 1, 2)


def clock(fn):
    """Host milliseconds of fn() up to the device having finished it."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pil_frames(n, raw_hw, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    return [Image.fromarray(rng.randint(0, 256, raw_hw + (3,), dtype=np.uint8)) for _ in range(n)]


def host_path(rgbs, out_hw, box, dev):
    """data.ScanNetFolder.__getitem__'s image lines (the KITTI loader crops where ScanNet's resizes), then the upload."""
    from PIL import Image
    from magnet_amd.data import IMAGENET_MEAN, IMAGENET_STD
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    imgs = []
    for rgb in rgbs:
        rgb = rgb.crop(box) if box is not None else rgb.resize((out_hw[1], out_hw[0]), resample=Image.BILINEAR)
        img = torch.from_numpy(np.asarray(rgb).astype(np.float32) / 255.0).permute(2, 0, 1)
        imgs.append((img - mean) / std)
    return torch.stack(imgs).to(dev)


def raw_frames(rgbs):
    """The raw_images=True lines: the decoded frames as one uint8 tensor."""
    return torch.stack([torch.from_numpy(np.array(rgb, dtype=np.uint8)) for rgb in rgbs])


def events_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


def med(xs):
    return round(statistics.median(xs), 4)


def part_ab(a, dev, parts):
    from magnet_amd import ingest
    for name, N, raw_hw, out_hw, kitti in SHAPES:
        prep = ingest.ImagePrep.kitti(raw_hw, device=dev) if kitti else ingest.ImagePrep(raw_hw, out_hw, device=dev)
        left, top, cw, ch = prep.crop
        box = (left, top, left + cw, top + ch) if kitti else None
        rgbs = pil_frames(N, raw_hw, seed=len(name))
        base = {"shape": name, "N": N, "raw_hw": list(raw_hw), "out_hw": list(out_hw), "crop": list(prep.crop), "gpu": torch.cuda.get_device_name(0)}
        sides = {"host": lambda: host_path(rgbs, out_hw, box, dev), "device": lambda: prep.prep(raw_frames(rgbs))}
        if "a" in parts:
            t = {k: [] for k in sides}
            outs = {}
            for i in range(a.warmup + a.pairs):
                for k in (("host", "device") if i % 2 == 0 else ("device", "host")):
                    ms, outs[k] = clock(sides[k])
                    if i >= a.warmup:
                        t[k].append(ms / N)
            emit({"bench": "ingest", "part": "a_end_to_end", **base, "pairs": a.pairs,
                  "host_ms_per_frame": [round(v, 4) for v in t["host"]], "device_ms_per_frame": [round(v, 4) for v in t["device"]],
                  "host_ms_per_frame_median": med(t["host"]), "device_ms_per_frame_median": med(t["device"]),
                  "pairs_won": {"host": sum(h < d for h, d in zip(t["host"], t["device"])), "device": sum(d < h for h, d in zip(t["host"], t["device"]))},
                  "upload_bytes_per_frame": {"host": 12 * out_hw[0] * out_hw[1], "device": 3 * raw_hw[0] * raw_hw[1]},
                  "differing_elements": int((outs["host"] != outs["device"]).sum())}, a.out)
        if "b" in parts:
            src = raw_frames(rgbs).to(dev)
            bytes_in, bytes_out = N * 3 * cw * ch, N * 3 * out_hw[0] * out_hw[1] * 4
            half = (bytes_in + bytes_out) // 2                      # a copy of `half` bytes reads and writes bytes_in + bytes_out in all
            sets = max(2, -(-a.ring_mb * 1000000 // (src.numel() + bytes_out)))
            k_src = [src.clone() for _ in range(sets)]
            k_out = [torch.empty((N, 3) + tuple(out_hw), device=dev) for _ in range(sets)]
            c_src = [torch.zeros(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            c_dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            turn = {"kernel": 0, "copy": 0}

            def kernel():
                i = turn["kernel"] = (turn["kernel"] + 1) % sets
                prep.prep(k_src[i], out=k_out[i])

            def copy():
                i = turn["copy"] = (turn["copy"] + 1) % sets
                c_dst[i].copy_(c_src[i])

            runs = {"kernel": kernel, "copy": copy}
            # eager launches include the host's time per call (the binding's checks cost more than a small launch runs), so each side's
            # walk once round its ring is also captured as a HIP graph: a replay is `sets` launches back to back with no host between
            graphs = {}
            for k, fn in runs.items():
                for _ in range(sets):
                    fn()
                torch.cuda.synchronize()
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k]):
                    for _ in range(sets):
                        fn()
            t = {k: [] for k in runs}
            eager = {k: [] for k in runs}
            for i in range(a.warmup + a.pairs):
                for k in (("kernel", "copy") if i % 2 == 0 else ("copy", "kernel")):
                    ms = events_ms(graphs[k].replay, 1) / sets
                    ms_eager = events_ms(runs[k], a.launches)
                    if i >= a.warmup:
                        t[k].append(ms)
                        eager[k].append(ms_eager)
            torch.cuda.synchronize()
            emit({"bench": "ingest", "part": "b_kernel", **base, "pairs": a.pairs, "launches_per_sample": a.launches, "buffer_sets": sets,
                  "bytes_in": bytes_in, "bytes_out": bytes_out,
                  "eager_kernel_us_median": round(statistics.median(eager["kernel"]) * 1e3, 2),
                  "eager_copy_us_median": round(statistics.median(eager["copy"]) * 1e3, 2),
                  "kernel_us": [round(v * 1e3, 2) for v in t["kernel"]], "copy_us": [round(v * 1e3, 2) for v in t["copy"]],
                  "kernel_us_median": round(statistics.median(t["kernel"]) * 1e3, 2), "copy_us_median": round(statistics.median(t["copy"]) * 1e3, 2),
                  "kernel_GB_per_s": round((bytes_in + bytes_out) / statistics.median(t["kernel"]) / 1e6, 1),
                  "copy_GB_per_s": round((bytes_in + bytes_out) / statistics.median(t["copy"]) / 1e6, 1),
                  "differing_elements": int((k_out[0] != k_out[sets - 1]).sum()),
                  "kernel_fraction_of_copy_rate": round(statistics.median(t["copy"]) / statistics.median(t["kernel"]), 3)}, a.out)


def part_c(a, dev):
    from magnet_amd import fnet, ingest, synth
    from magnet_amd.magnet import MAGNET
    from magnet_amd.sequence import SequenceRunner
    from magnet_amd.standin import make_args, make_dnet, seeded_magnet_weights
    wl = synth.WORKLOADS["C2"]
    h, w, V = wl.h, wl.w, 4
    out_hw, raw_hw = (4 * h, 4 * w), (968, 1296)
    args = make_args(D=wl.D, iters=wl.iters, dpv_h=h, dpv_w=w, fdim=64, V=V)
    args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
    model = MAGNET(args, d_net=make_dnet(backend="hip"), f_net=fnet.FNET(args), feat_dtype=wl.feat_dtype, dnet_backend="hip").to(dev).eval()
    seeded_magnet_weights(model, seed=4)
    rgbs = pil_frames(8, raw_hw, seed=2)                            # 8 distinct frames, walked cyclically under ever new ids
    intr = synth.make_intrinsics(wl.camera, h, w, 1)
    valid = torch.ones(1, V, dtype=torch.int32)
    g = torch.Generator().manual_seed(1)
    for graph in (False, True):
        prep = ingest.ImagePrep(raw_hw, out_hw, device=dev)
        runners = {"host": SequenceRunner(model, 8, graph=graph), "device": SequenceRunner(model, 8, graph=graph, image_prep=prep)}
        t = {k: [] for k in runners}
        diffs = []
        with torch.no_grad():
            runners["host"].add(list(range(4)), host_path(rgbs[:4], out_hw, None, dev))
            runners["device"].add(list(range(4)), raw_frames(rgbs[:4]))
            for step in range(a.warmup + a.pairs):
                tt = 4 + step
                rgb = [rgbs[tt % 8]]
                refs, nghbrs = [tt - 2], [tt - 2 + o for o in OFFSETS]
                poses = synth.make_poses(wl.camera, 1, V, g).to(dev)
                steps = {"host": lambda: (runners["host"].add([tt], host_path(rgb, out_hw, None, dev)), runners["host"].refine(refs, nghbrs, poses, valid, intr))[1],
                         "device": lambda: (runners["device"].add([tt], raw_frames(rgb)), runners["device"].refine(refs, nghbrs, poses, valid, intr))[1]}
                outs = {}
                for k in (("host", "device") if step % 2 == 0 else ("device", "host")):
                    ms, outs[k] = clock(steps[k])
                    if step >= a.warmup:
                        t[k].append(ms)
                diffs.append(float((outs["host"][-1] - outs["device"][-1]).abs().max()))
        emit({"bench": "ingest", "part": "c_pool_reuse", "config": "C2", "graph": graph, "raw_hw": list(raw_hw), "out_hw": list(out_hw), "B": 1, "V": V,
              "pairs": a.pairs, "gpu": torch.cuda.get_device_name(0),
              "host_ms_per_step": [round(v, 3) for v in t["host"]], "device_ms_per_step": [round(v, 3) for v in t["device"]],
              "host_ms_per_step_median": med(t["host"]), "device_ms_per_step_median": med(t["device"]),
              "pairs_won": {"host": sum(x < y for x, y in zip(t["host"], t["device"])), "device": sum(y < x for x, y in zip(t["host"], t["device"]))},
              "frames_prepared": runners["device"].prepared, "max_abs_diff_last_prediction": max(diffs)}, a.out)
        del runners


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20, help="(b): launches between the two HIP events of one sample")
    ap.add_argument("--ring_mb", type=int, default=640, help="(b): total size of the ring of buffer sets each side walks")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py needs an MI355X (no CPU fallback)")
    from magnet_amd import lib
    lib.load()
    dev = torch.device("cuda:0")
    parts = a.parts.split(",")
    if "a" in parts or "b" in parts:
        part_ab(a, dev, parts)
    if "c" in parts:
        part_c(a, dev)


if __name__ == "__main__":
    main()
