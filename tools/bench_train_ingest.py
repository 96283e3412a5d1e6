"""Training-sample preparation, host path against device path (magnet_amd/ingest.py: TrainPrep; magnet_train_prep_u8,
magnet_depth_prep_u16).  One process on one MI355X, one CPU thread.  The sibling of tools/bench_ingest.py, whose helpers it uses: both
sides start from decoded frames and depth maps (decoding is the same work on both sides and is left out) and end with the fp32
tensors on the device, the device idle.  Every sample carries a colour draw, the single-view one also a flip and a crop window.

  (a) per shape, --pairs interleaved pairs, the side that goes first alternating:
        host    the training loaders' lines: Pillow BILINEAR / NEAREST resize, flip, numpy fp32 / 255 and / 1000, crop window,
                data.augment_image, torch (x - mean) / std, stack, .to(device) of the fp32 tensors
        device  np.array into uint8 / uint16 tensors, stack, TrainPrep.params (one upload), prep, prep_depth (one launch each)
      ms per sample of both, pairs won, and the outputs compared (differing elements: 0).
  (b) magnet_image_prep_u8's kernel alone, this build against the library of another commit (--other_lib PATH, a libmagnet_hip.so
      built from it), at bench_ingest's three shapes: the same argument struct handed to both libraries, one walk round a ring of
      buffer sets (--ring_mb, beyond the last-level cache) replayed as a HIP graph, interleaved pairs; the other library's own
      pair-to-pair spread is reported beside the difference.
  (c) both new kernels alone (tables and records already uploaded) against a device-to-device copy of the same total bytes, as
      bench_ingest's part (b).

    python tools/bench_train_ingest.py [--pairs 12] [--warmup 3] [--parts a,b,c] [--other_lib PATH] [--out profiles/train_ingest/bench.jsonl]
"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_ingest import SHAPES as INFERENCE_SHAPES, clock, emit, events_ms, med, pil_frames, raw_frames  # noqa: E402

COLOR = (0.95, 1.2, (1.05, 0.93, 1.08))
# name, samples, frames per sample, raw (H, W), depth raw (H, W), resized (H, W), window (H, W) or None, flip, window origin (x, y)
SHAPES = (("multi_view_1", 1, 5, (968, 1296), (480, 640), (480, 640), None, False, None),
          ("multi_view_4", 4, 5, (968, 1296), (480, 640), (480, 640), None, False, None),
          ("single_view_1", 1, 1, (968, 1296), (480, 640), (480, 640), (416, 544), True, (40, 30)))


def pil_depths(n, hw, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    return [Image.fromarray(rng.randint(0, 10000, hw).astype(np.uint16)) for _ in range(n)]


def host_path(rgbs, depths, res_hw, out_hw, flip, origin, dev):
    """The training loaders' lines (data.ScanNetFolder(augment=...) / data.ScanNetFrames), then the upload."""
    from PIL import Image
    from magnet_amd.data import IMAGENET_MEAN, IMAGENET_STD, augment_image
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    x, y = origin or (0, 0)
    h, w = out_hw or res_hw
    imgs, gts = [], []
    for rgb in rgbs:
        rgb = rgb.resize((res_hw[1], res_hw[0]), resample=Image.BILINEAR)
        if flip:
            rgb = rgb.transpose(Image.FLIP_LEFT_RIGHT)
        img = np.array(rgb).astype(np.float32) / 255.0
        img = augment_image(img[y:y + h, x:x + w, :], *COLOR)
        imgs.append((torch.from_numpy(img).permute(2, 0, 1) - mean) / std)
    for dm in depths:
        if (dm.height, dm.width) != tuple(res_hw):
            dm = dm.resize((res_hw[1], res_hw[0]), resample=Image.NEAREST)
        if flip:
            dm = dm.transpose(Image.FLIP_LEFT_RIGHT)
        d = np.array(dm)[:, :, np.newaxis].astype(np.float32) / 1000.0
        gts.append(torch.from_numpy(np.ascontiguousarray(d[y:y + h, x:x + w, :])).permute(2, 0, 1))
    return torch.stack(imgs).to(dev), torch.stack(gts).to(dev)


def device_path(prep, rgbs, depths, augs, per_sample):
    frames = raw_frames(rgbs)
    maps = torch.stack([torch.from_numpy(np.array(dm, dtype=np.uint16)) for dm in depths])
    p = prep.params(augs)                                         # frame-major, as collate stacks a batch: the reference frames' records are
    first = (per_sample // 2) * len(depths)                       # one contiguous run of the upload
    return prep.prep(frames, p), prep.prep_depth(maps, p[first:first + len(depths)])


def part_a(a, dev):
    from magnet_amd import ingest
    from magnet_amd.data import Augment
    for name, S, F, raw_hw, depth_hw, res_hw, out_hw, flip, origin in SHAPES:
        prep = ingest.TrainPrep(raw_hw, res_hw, out_hw=out_hw, device=dev)
        rgbs, depths = pil_frames(S * F, raw_hw, seed=len(name)), pil_depths(S, depth_hw, seed=S)
        augs = [Augment(COLOR, flip, origin)] * (S * F)
        sides = {"host": lambda: host_path(rgbs, depths, res_hw, out_hw, flip, origin, dev),
                 "device": lambda: device_path(prep, rgbs, depths, augs, F)}
        t, outs = {k: [] for k in sides}, {}
        for i in range(a.warmup + a.pairs):
            for k in (("host", "device") if i % 2 == 0 else ("device", "host")):
                ms, outs[k] = clock(sides[k])
                if i >= a.warmup:
                    t[k].append(ms / S)
        emit({"bench": "train_ingest", "part": "a_end_to_end", "shape": name, "samples": S, "frames_per_sample": F, "raw_hw": list(raw_hw),
              "depth_hw": list(depth_hw), "resize_hw": list(res_hw), "out_hw": list(out_hw or res_hw), "flip": flip, "pairs": a.pairs,
              "gpu": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
              "host_ms_per_sample": [round(v, 3) for v in t["host"]], "device_ms_per_sample": [round(v, 3) for v in t["device"]],
              "host_ms_per_sample_median": med(t["host"]), "device_ms_per_sample_median": med(t["device"]),
              "pairs_won": {"host": sum(h < d for h, d in zip(t["host"], t["device"])), "device": sum(d < h for h, d in zip(t["host"], t["device"]))},
              "differing_elements": [int((h.view(torch.int32) != d.view(torch.int32)).sum()) for h, d in zip(outs["host"], outs["device"])]}, a.out)


def replayed(runs, sets, a):
    """{name: fn} -> {name: [ms per launch of each timed pair]}: each fn's walk once round its ring captured as a HIP graph, the graphs
    replayed in interleaved order."""
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
    names = list(runs)
    for i in range(a.warmup + a.pairs):
        for k in (names if i % 2 == 0 else names[::-1]):
            ms = events_ms(graphs[k].replay, 1) / sets
            if i >= a.warmup:
                t[k].append(ms)
    torch.cuda.synchronize()
    return t


def part_b(a, dev):
    """The inference kernel of this build against --other_lib's, through the C ABI itself (no binding code in the timed path)."""
    from magnet_amd import ingest, lib
    libs = {"this": lib.load(), "other": ctypes.CDLL(os.path.abspath(a.other_lib))}
    for L in libs.values():
        L.magnet_image_prep_u8.restype, L.magnet_image_prep_u8.argtypes = lib._PROTOS["magnet_image_prep_u8"]
    for name, N, raw_hw, out_hw, kitti in INFERENCE_SHAPES:
        prep = ingest.ImagePrep.kitti(raw_hw, device=dev) if kitti else ingest.ImagePrep(raw_hw, out_hw, device=dev)
        left, top, cw, ch = prep.crop
        src = raw_frames(pil_frames(N, raw_hw, seed=len(name))).to(dev)
        bytes_out = N * 3 * out_hw[0] * out_hw[1] * 4
        sets = max(2, -(-a.ring_mb * 1000000 // (src.numel() + bytes_out)))
        srcs = [src.clone() for _ in range(sets)]
        outs = {k: [torch.zeros((N, 3) + tuple(out_hw), device=dev) for _ in range(sets)] for k in libs}
        tx, ty, lut = prep.tables()
        structs = {k: [] for k in libs}
        for k in libs:
            for i in range(sets):
                s = lib.MagnetImagePrepArgs(src=srcs[i].data_ptr(), src_pitch=srcs[i].stride(1), src_frame=srcs[i].stride(0), lut=lut.data_ptr(),
                                            out=outs[k][i].data_ptr(), N=N, Hin=raw_hw[0], Win=raw_hw[1], crop_left=left, crop_top=top, crop_w=cw,
                                            crop_h=ch, Hout=out_hw[0], Wout=out_hw[1])
                for axis, tab in (("x", tx), ("y", ty)):
                    if tab is not None:
                        setattr(s, "coef_" + axis, tab[0].data_ptr()); setattr(s, "bounds_" + axis, tab[1].data_ptr()); setattr(s, "k" + axis, int(tab[0].shape[1]))
                structs[k].append(s)
        turn = {k: 0 for k in libs}

        def run(k):
            def fn():
                i = turn[k] = (turn[k] + 1) % sets
                rc = libs[k].magnet_image_prep_u8(ctypes.byref(structs[k][i]), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
            return fn

        # "other" twice: the spread between two graphs of the same library is the bar for the difference between the two libraries
        t = replayed({"this": run("this"), "other": run("other"), "other_again": run("other")}, sets, a)
        us = {k: [round(v * 1e3, 2) for v in vs] for k, vs in t.items()}
        emit({"bench": "train_ingest", "part": "b_inference_kernel_this_vs_other", "shape": name, "N": N, "pairs": a.pairs, "buffer_sets": sets,
              "gpu": torch.cuda.get_device_name(0), **{k + "_us": v for k, v in us.items()}, **{k + "_us_median": med(v) for k, v in us.items()},
              "this_minus_other_us": [round(x - y, 2) for x, y in zip(us["this"], us["other"])],
              "other_again_minus_other_us": [round(x - y, 2) for x, y in zip(us["other_again"], us["other"])],
              "pairs_this_faster": sum(x < y for x, y in zip(us["this"], us["other"])),
              "differing_elements": int((outs["this"][0] != outs["other"][0]).sum())}, a.out)


def part_c(a, dev):
    from magnet_amd import ingest
    from magnet_amd.data import Augment
    for name, S, F, raw_hw, depth_hw, res_hw, out_hw, flip, origin in SHAPES:
        prep = ingest.TrainPrep(raw_hw, res_hw, out_hw=out_hw, device=dev)
        h, w = out_hw or res_hw
        N = S * F
        p = prep.params([Augment(COLOR, flip, origin)] * N)
        frames = raw_frames(pil_frames(N, raw_hw, seed=len(name))).to(dev)
        maps = torch.stack([torch.from_numpy(np.array(dm, dtype=np.uint16)) for dm in pil_depths(S, depth_hw, seed=S)]).to(dev)
        for kind, src, n, ch, recs in (("train_prep_u8", frames, N, 3, p), ("depth_prep_u16", maps, S, 1, p[:S])):
            bytes_in, bytes_out = src.numel() * src.element_size(), n * ch * h * w * 4
            half = (bytes_in + bytes_out) // 2
            sets = max(2, -(-a.ring_mb * 1000000 // (bytes_in + bytes_out)))
            k_src = [src.clone() for _ in range(sets)]
            k_out = [torch.empty((n, ch, h, w), device=dev) for _ in range(sets)]
            c_src = [torch.zeros(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            c_dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            turn = {"kernel": 0, "copy": 0}
            call = prep.prep if ch == 3 else prep.prep_depth

            def kernel():
                i = turn["kernel"] = (turn["kernel"] + 1) % sets
                call(k_src[i], recs, out=k_out[i])

            def copy():
                i = turn["copy"] = (turn["copy"] + 1) % sets
                c_dst[i].copy_(c_src[i])

            t = replayed({"kernel": kernel, "copy": copy}, sets, a)
            emit({"bench": "train_ingest", "part": "c_kernel", "kernel": kind, "shape": name, "N": n, "pairs": a.pairs, "buffer_sets": sets,
                  "bytes_in": bytes_in, "bytes_out": bytes_out, "gpu": torch.cuda.get_device_name(0),
                  "kernel_us": [round(v * 1e3, 2) for v in t["kernel"]], "copy_us": [round(v * 1e3, 2) for v in t["copy"]],
                  "kernel_us_median": round(statistics.median(t["kernel"]) * 1e3, 2), "copy_us_median": round(statistics.median(t["copy"]) * 1e3, 2),
                  "kernel_fraction_of_copy_rate": round(statistics.median(t["copy"]) / statistics.median(t["kernel"]), 3)}, a.out)
            del k_src, k_out, c_src, c_dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ring_mb", type=int, default=640, help="(b), (c): total size of the ring of buffer sets each side walks")
    ap.add_argument("--parts", default="a,c")
    ap.add_argument("--other_lib", default=None, help="(b): a libmagnet_hip.so built from another commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_ingest.py needs an MI355X (no CPU fallback)")
    torch.set_num_threads(1)
    from magnet_amd import lib
    lib.load()
    dev = torch.device("cuda:0")
    parts = a.parts.split(",")
    if "a" in parts:
        part_a(a, dev)
    if "b" in parts:
        if not a.other_lib:
            raise SystemExit("part b compares against --other_lib PATH")
        part_b(a, dev)
    if "c" in parts:
        part_c(a, dev)


if __name__ == "__main__":
    main()
