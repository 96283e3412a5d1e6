"""Evaluation over ranks: every rank runs its contiguous share of the loader's batches into a device MetricTable (metrics.py), the
per-frame rows are gathered once, and every rank replays the reference's running average over them in loader order - so the 12
numbers are the single-process loop's to the bit, whatever the world size ("optional gather of per-frame
metrics").  gather_rows() is the only call of an evaluation that waits for the device."""
from __future__ import annotations

import json
import os
import sys

import torch
import torch.distributed as tdist

from . import dist as mdist
from .metrics import METRIC_ORDER


def shard_batches(loader, rank: int = 0, world: int = 1):
    """The batches of `loader` whose index lies in dist.shard_range(len(loader), rank, world).  The loader is iterated from its start
    and the batches of other ranks are skipped, so a seeded generator loader yields, batch for batch, what the unsharded loop sees;
    sharding by batch keeps every batch's composition independent of the world size."""
    lo, hi = mdist.shard_range(len(loader), rank, world)
    if hi <= lo:
        return
    for i, batch in enumerate(loader):
        if i >= hi:
            break
        if i >= lo:
            yield batch


def gather_rows(rows: torch.Tensor) -> torch.Tensor:
    """Every rank's (n_r, 12) float64 rows as one CPU tensor, concatenated in rank order (= loader order).  One all-gather of the
    counts, one all-gather of the rows padded to the largest count; device tensors under nccl, CPU tensors under gloo.  Without a
    process group: rows.cpu()."""
    if not (tdist.is_available() and tdist.is_initialized()):
        return rows.detach().cpu()
    world = tdist.get_world_size()
    rows = rows.detach() if tdist.get_backend() == "nccl" else rows.detach().cpu()
    count = torch.tensor([rows.shape[0]], dtype=torch.int64, device=rows.device)
    counts = [torch.zeros_like(count) for _ in range(world)]
    tdist.all_gather(counts, count)
    counts = [int(c) for c in torch.cat(counts).tolist()]
    padded = torch.zeros((max(max(counts), 1), rows.shape[1]), dtype=rows.dtype, device=rows.device)
    padded[:rows.shape[0]].copy_(rows)
    parts = [torch.empty_like(padded) for _ in range(world)]
    tdist.all_gather(parts, padded)
    return torch.cat([p[:n] for p, n in zip(parts, counts)]).cpu()


def running_average(rows) -> dict:
    """metrics.RunningAverage's update, avg = (value + count * avg) / (count + 1), replayed over the rows in order in Python floats:
    the value the per-frame loops arrive at, to the bit, NaN propagation included.  No rows: every metric is NaN."""
    avg = [0] * len(METRIC_ORDER)
    count = 0
    for row in (rows.tolist() if isinstance(rows, torch.Tensor) else rows):
        avg = [(value + count * a) / (count + 1) for value, a in zip(row, avg)]
        count += 1
    if count == 0:
        return {k: float("nan") for k in METRIC_ORDER}
    return dict(zip(METRIC_ORDER, avg))


def evaluate(step, loader, table, rank: int = 0, world: int = 1):
    """Run step(batch) - which appends the batch's frames to `table` - over this rank's batches, then gather the rows and average on
    every rank.  Returns (metric dict, number of frames)."""
    for batch in shard_batches(loader, rank, world):
        step(batch)
    rows = gather_rows(table.rows())
    return running_average(rows), int(rows.shape[0])


# ---- what the three evaluation drivers share: the flags, the launch and the result file ----
def add_arguments(ap):
    ap.add_argument("--sharded", action="store_true",
                    help="run validate_sharded(): metric rows stay on the device, one gather at the end (implied by more than one rank)")
    ap.add_argument("--gpus", type=int, default=1, help="start this many ranks of this command line (dist.spawn_ranks), one share of the batches each")
    ap.add_argument("--dist_backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend; gloo gathers through the host and lets several ranks share one GPU")
    ap.add_argument("--dump_metrics", default="", help="with --sharded: write the 12 metrics as float.hex() strings and the frame count to this JSON file")


def start(a, script):
    """-> (rank, world, device, sharded).  `--gpus N` outside a launcher starts the N ranks as child processes and exits with their
    return code; under a launcher (RANK set: torch.distributed.run or our own spawn) the process joins the group."""
    launched = "RANK" in os.environ
    if a.gpus > 1 and not launched:
        raise SystemExit(mdist.spawn_ranks(a.gpus, [os.path.abspath(script)] + sys.argv[1:]))
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(script)} needs an MI355X (no CPU fallback)")
    rank, world, local = mdist.env_world() if launched else (0, 1, 0)
    n_dev = torch.cuda.device_count()
    if launched:
        if a.dist_backend == "nccl" and (int(os.environ.get("LOCAL_WORLD_SIZE", 0)) or world) > n_dev:
            raise SystemExit(f"{world} ranks on {n_dev} GPU(s): nccl needs one GPU per rank; use --dist_backend gloo to share GPUs")
        mdist.init_from_env(backend=a.dist_backend)
    device = torch.device("cuda", local % n_dev)
    torch.cuda.set_device(device)
    sharded = a.sharded or world > 1
    if a.dump_metrics and not sharded:
        raise SystemExit("--dump_metrics needs --sharded")
    return rank, world, device, sharded


def dump_metrics(path, metrics, n_frames):
    """The result as exact text: {"frames": n, "metrics": {name: float.hex(value)}} in METRIC_ORDER."""
    with open(path, "w") as f:
        json.dump({"frames": int(n_frames), "metrics": {k: float(metrics[k]).hex() for k in METRIC_ORDER}}, f, indent=1)
        f.write("\n")


def finish():
    if tdist.is_available() and tdist.is_initialized():
        tdist.barrier()
        tdist.destroy_process_group()
