"""The evaluation loops, per-batch read-back against the device metric table: validate() and validate_sharded(world 1) of
eval_synthetic.py and eval_dnet.py at 480 x 640, batch 1, 64 frames, alternated in pairs in one process after a warm-up.  Every run
ends in torch.cuda.synchronize(); the wall time per frame of both and the number of host synchronisations per batch (the calls that
torch's sync debug mode flags, counted in a separate untimed run of each loop) go out as one JSON line per configuration and data
placement.  The frames are generated once and replayed from a list, from host memory (the loaders' case: every batch is uploaded
inside the loop) and from device memory (the loop alone).

    python tools/bench_eval.py [--pairs 8] [--frames 64] [--out lines.jsonl]
"""
import argparse
import json
import os
import sys
import time
import warnings

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

import torch  # noqa: E402

H, W = 480, 640


def _to(x, dev):
    if isinstance(x, torch.Tensor):
        return x.to(dev)
    if isinstance(x, dict):
        return {k: _to(v, dev) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to(v, dev) for v in x)
    return x


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _syncs(fn):
    """Synchronising calls torch's sync debug mode flags while fn runs."""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message) for w in rec)


def _configs(dev, frames):
    import eval_dnet
    import eval_synthetic
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import StubDNet, StubFNet, make_args, make_dnet, seeded_magnet_weights
    args = make_args(D=5, iters=3, dpv_h=H // 4, dpv_w=W // 4, V=4)                     # eval_synthetic.py's defaults
    args.min_depth, args.max_depth, args.garg_crop, args.eigen_crop = 1e-3, 10.0, False, False
    model = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2), feat_dtype="fp32")
    seeded_magnet_weights(model, 3)
    model = model.to(dev).eval()
    yield ("eval_synthetic", list(eval_synthetic.SyntheticWindows(frames, 1, 4, H, W, nan_every=3)),
           lambda ld: eval_synthetic.validate(model, args, ld, dev), lambda ld: eval_synthetic.validate_sharded(model, args, ld, dev))
    dargs = argparse.Namespace(min_depth=1e-3, max_depth=10.0, garg_crop=False, eigen_crop=False)
    dnet = make_dnet(dnet=True, backend="hip").to(dev).eval()
    yield ("eval_dnet", list(eval_dnet.SyntheticFrames(frames, 1, H, W)),
           lambda ld: eval_dnet.validate(dnet, dargs, ld, dev), lambda ld: eval_dnet.validate_sharded(dnet, dargs, ld, dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8); ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from magnet_amd import metrics as M
    lines = []
    for name, batches, old, new in _configs(dev, a.frames):
        for place in ("host", "device"):
            ld = batches if place == "host" else _to(batches, dev)
            for _ in range(2):                                                          # warm-up: library load, allocator, clocks
                m_old, m_new = old(ld), new(ld)
            pairs = []
            for _ in range(a.pairs):
                t_old, _ = _timed(lambda: old(ld))
                t_new, _ = _timed(lambda: new(ld))
                pairs.append((t_old / a.frames * 1e3, t_new / a.frames * 1e3))
            line = {"config": name, "H": H, "W": W, "batch": 1, "frames": a.frames, "data": place,
                    "ms_per_frame_validate": [round(p[0], 4) for p in pairs],
                    "ms_per_frame_validate_sharded": [round(p[1], 4) for p in pairs],
                    "pairs_where_sharded_is_slower": sum(p[1] > p[0] for p in pairs),
                    "syncs_per_batch_validate": _syncs(lambda: old(ld)) / a.frames,
                    "syncs_per_batch_validate_sharded": _syncs(lambda: new(ld)) / a.frames,
                    "values_differ": sorted(k for k in M.METRIC_ORDER if float(m_old[k]).hex() != float(m_new[k]).hex()),
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del ld
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
