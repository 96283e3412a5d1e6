#!/usr/bin/env python3
"""bench.py — MaGNet multi-view matching hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]     (N>1: launched by torch.distributed.run)

One STEP = one pass of the hot path (models/MAGNET.py:146-175) over a batch of `--frames`
reference frames per GPU, starting from backbone outputs already resident in HBM:
    pack F-Net features (NCHW fp32 -> channel-last) -> I x [fused sample+warp+score kernel ->
    G-Net convs -> Gaussian update] -> mask head -> convex upsampling -> list of (B,2,H,W).
Workload (default C2 = BASELINE.json configs[1]): ScanNet 480x640 input -> 120x160 matching grid,
V=4 source views, D=64 candidates, F=64, I=1, bf16-stored features, synthetic tensors.
Frames shard across ranks with no data-path collective (weak scaling: per-GPU work is fixed);
the only collective is a one-time RCCL broadcast of G-Net/mask-head weights.

Prints ONE JSON line on rank 0 (fields: see the task contract).  A plain run sets up, warms up, times the K steps and prints the
headline (`value`, `ms_per_step`); --dump-outputs DIR also writes what the last timed step returned as DIR/<name>.npy.
--full adds everything else the line carries, each measured in passes of its own after the timed steps:
  roofline      — fused cost-volume kernel: algorithmic bytes per launch / HIP-event time per launch, live rocprofv3 counters
  roofline_conv — the 3x3 convolution launches against the matrix-core peak
  sustained_frames_per_s, ms_per_step_inputs_in_kernel_layouts — the step run on for --sustain-s seconds / without its pack passes
  cpu_baseline  — the CPU oracle (oracle/, a restatement of the reference validated against it)
                  timed on this host's cores on a bounded sample of the same workload (rank 0, N=1)
  rccl          — at N=1 too: a one-rank process group, the weight broadcast (with the F-Net bucket) and its verification
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from magnet_amd import dist as mdist  # noqa: E402
from magnet_amd import synth  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy rate
DUMP_BUDGET_BYTES = 60 * 10**6  # --dump-outputs stays under 64 MB in all, .npy headers included


class _NoBackbone(torch.nn.Module):
    """D-Net / F-Net are out of scope; the bench starts from their outputs."""

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("bench.py feeds backbone outputs directly (match_and_refine)")


def make_args(wl, iters):
    from types import SimpleNamespace
    return SimpleNamespace(MAGNET_sampling_range=3, MAGNET_num_samples=wl.D, MAGNET_mvs_weighting="CW5",
                           MAGNET_num_train_iter=iters, MAGNET_num_test_iter=iters,
                           MAGNET_num_source_views=wl.V, dpv_height=wl.h, dpv_width=wl.w, downsample_ratio=4,
                           FNET_feature_dim=wl.F, DNET_ckpt=None, FNET_ckpt=None, MAGNET_ckpt=None)


def device_inputs(wl, B, seed, device):
    """Synthetic backbone outputs generated directly on the GPU (distributions of SURVEY.md §8d)."""
    g = torch.Generator(device=device).manual_seed(seed)
    cam = synth.CAMERAS[wl.camera]
    h, w, V, F = wl.h, wl.w, wl.V, wl.F
    rnd = lambda *s: torch.randn(*s, generator=g, device=device)
    uni = lambda lo, hi, *s: torch.rand(*s, generator=g, device=device) * (hi - lo) + lo
    ref_feat, src_feat = rnd(B, F, h, w), rnd(V * B, F, h, w)
    gmm = lambda n: torch.cat([uni(*cam["mu"], n, 1, h, w), uni(*cam["sigma"], n, 1, h, w)], dim=1)
    cpu_gen = torch.Generator().manual_seed(seed)
    return dict(ref_feat=ref_feat, nghbr_feat=src_feat, ref_gmms=gmm(B), nghbr_gmms=gmm(V * B),
                x_d3=rnd(B, 256, h, w) * 0.5,
                nghbr_poses=synth.make_poses(wl.camera, B, V, cpu_gen).to(device),
                is_valid=torch.ones(B, V, dtype=torch.int32),
                cam_intrins=synth.make_intrinsics(wl.camera, h, w, B))


def dump_outputs(out, dirname, seed=0):
    """Write what one step returned as dirname/<name>.npy (float32): a list of predictions as pred_<i>, a dict under its keys.  When
    the whole exceeds DUMP_BUDGET_BYTES every array keeps the same seeded share of itself: whole slices along its first dimension
    (frames of a prediction) where at least one fits, else single elements.  The sample depends on the shapes and `seed` only, so
    two runs with the same arguments write the same positions."""
    import numpy as np
    arrays = out if isinstance(out, dict) else {f"pred_{i}": t for i, t in enumerate(out)}
    frac = min(1.0, DUMP_BUDGET_BYTES / max(1, sum(t.numel() * 4 for t in arrays.values())))
    os.makedirs(dirname, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        if frac < 1.0:
            rng = np.random.default_rng(seed)
            keep = int(t.shape[0] * frac)
            if keep >= 1:
                idx = np.sort(rng.choice(t.shape[0], keep, replace=False))
                t = t.index_select(0, torch.from_numpy(idx).to(t.device))
            else:
                idx = np.sort(rng.choice(t.numel(), max(1, int(t.numel() * frac)), replace=False))
                t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(dirname, f"{name}.npy"), t.float().cpu().numpy())
    return sorted(arrays)


def _cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown CPU"


def cpu_baseline(wl, model_cpu, iters, budget_s=10.0):
    """The hot path on the host CPU: oracle matcher (OpenMP) + torch-CPU G-Net + oracle tail / upsample.
    Bounded and reproducible: every figure is taken AFTER a warm-up call (the OpenMP team and the page cache exist) and the
    matcher-only figures are medians of >= 5 (all cores) / 3 (batched) calls; a 1-thread matcher call and the CPU model string
    are reported as SURVEY.md section 8d asks."""
    import statistics
    from oracle import oracle
    cores = oracle.num_threads()
    torch.set_num_threads(cores)
    k = oracle.depth_sampling(3, wl.D)
    inp = synth.make_inputs(wl, B=1, seed=0)
    x_d3 = torch.randn(1, 256, wl.h, wl.w, generator=torch.Generator().manual_seed(1)) * 0.5

    def matcher(i, gmm, nthr):
        return oracle.cost_volume_cw(None, gmm, k, i["ref_feat"], i["nghbr_feat"], i["nghbr_gmms"], i["nghbr_poses"],
                                     i["is_valid"], i["cam_intrins"]["intM"], i["cam_intrins"]["unit_ray_array_2D"], 5.0,
                                     n_threads=nthr)

    def one_frame():
        gmm = inp["ref_gmms"].clone()
        with torch.no_grad():
            for _ in range(iters):
                cost = torch.from_numpy(matcher(inp, gmm, cores))
                raw = model_cpu.g_net.gnet(torch.cat([cost, x_d3], dim=1))
                gmm = torch.from_numpy(oracle.gaussian_update(raw.numpy(), gmm.numpy()))
            mask = model_cpu.mask_head(x_d3)
            oracle.upsample_depth_via_mask(gmm.numpy(), mask.numpy(), 4)

    def timed(fn):
        t0 = time.perf_counter(); fn(); return time.perf_counter() - t0

    one_frame()                                              # warm-up: thread teams, allocator, page cache
    t1 = timed(one_frame)
    n = max(2, min(64, int(budget_s / max(t1, 1e-3))))
    dt = timed(lambda: [one_frame() for _ in range(n)])
    # matcher only, for the kernel-level comparison: median of 5 warmed calls on one frame (all cores) ...
    tm = statistics.median(timed(lambda: matcher(inp, inp["ref_gmms"], cores)) for _ in range(5))
    # ... the CPU's best case, a batch of frames in one call (the OpenMP loop runs over frame x row) ...
    nb = 8
    inb = synth.make_inputs(wl, B=nb, seed=0)
    matcher(inb, inb["ref_gmms"], cores)
    tb = statistics.median(timed(lambda: matcher(inb, inb["ref_gmms"], cores)) for _ in range(3))
    # ... and one thread (one frame, one call after the warm-up above)
    t_1 = timed(lambda: matcher(inp, inp["ref_gmms"], 1))
    matcher(inp, inp["ref_gmms"], cores)                      # leave the OpenMP team size as found
    return {"value": n / dt, "unit": "ref-frames/s", "cores": cores, "kind": "port", "cpu_model": _cpu_model(),
            "sample": f"{n} frame(s) of {wl.name} ({wl.h}x{wl.w} grid, V={wl.V}, D={wl.D}, I={iters}) after one warm-up frame, "
                      f"{dt:.1f} s wall; oracle matcher OpenMP x{cores} + torch-CPU G-Net/mask head x{cores}; host CPU: {_cpu_model()}",
            "matcher_only_frames_per_s": 1.0 / tm,
            "matcher_only_batched_frames_per_s": nb / tb,
            "matcher_only_1_thread_frames_per_s": 1.0 / t_1,
            "matcher_only_sample": f"median of 5 warmed calls on 1 frame x{cores} threads; median of 3 warmed calls on {nb} frames "
                                   f"x{cores} threads; 1 call on 1 frame x1 thread"}


def _child_env(environ=None) -> dict:
    """A clean single-process environment for a counter-pass child of this script: under torchrun the parent's rendezvous variables
    (and TORCHELASTIC_USE_AGENT_STORE, which makes env:// rendezvous a CLIENT of the agent's store) would make the child's own one-rank
    group wait for a store that does not exist until the pass times out."""
    environ = os.environ if environ is None else environ
    env = {k_: v_ for k_, v_ in environ.items()
           if not (k_.startswith(("TORCHELASTIC_", "TORCH_NCCL_", "GROUP_", "ROLE_")) or
                   k_ in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"))}
    env["TMPDIR"] = "/tmp"
    return env


def _pmc_passes(passes, child_args, kernel_match, timeout_s=90):
    """One rocprofv3 --kernel-trace --pmc child run of this script per counter group (the guide: counters in their own runs, never
    combined with tracing domains other than the kernel trace).  Returns {counter: mean per dispatch} over the dispatches whose kernel
    name `kernel_match` accepts, plus "_ns" = their mean duration; {} for a group whose pass failed."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    vals = {}
    if shutil.which("rocprofv3") is None:
        return vals
    for tag, ctrs in passes.items():
        tmp = tempfile.mkdtemp(prefix="magnet_pmc_", dir="/tmp")
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", *ctrs, "--output-format", "csv", "-d", tmp, "-o", "p", "--",
               sys.executable, os.path.abspath(__file__), "--full", "--no-pmc", "--no-cpu-baseline", "--sustain-s", "0", *child_args]
        try:
            env = _child_env()
            # own session: on a timeout the whole group (profiler + the python it started) is stopped, not only the profiler
            pr = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc_ = pr.wait(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                import signal
                os.killpg(pr.pid, signal.SIGKILL)
                pr.wait()
                raise
            if rc_ != 0:
                raise RuntimeError(f"rocprofv3 exited with {rc_}")
            acc, dur = {}, []
            for f in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if kernel_match(r["Kernel_Name"]):
                        acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
                        dur.append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
            for c_, v_ in acc.items():
                vals[c_ if c_ not in vals else f"{c_}@{tag}"] = sum(v_) / len(v_)
            if dur:
                vals[f"_ns@{tag}"] = sum(dur) / len(dur)
        except Exception as e:                                   # profiler missing / hung / refused: report nothing rather than a stale number
            print(f"[bench] rocprofv3 pass {tag} failed ({type(e).__name__}); its counters are omitted", file=sys.stderr)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return vals


def live_counters(wl, B, fdt, timeout_s=90, path=0, dev_lib=False):
    """rocprofv3 --kernel-trace --pmc passes (FETCH_SIZE, WRITE_SIZE, SQ instruction counters, address-unit busy: separate runs, as
    the guide prescribes) over `bench.py --kernel-only` of the same workload, in child processes.  HBM bytes per launch =
    FETCH_SIZE [KB] x 1024 x 2.0 (gfx950 tallies 128-byte read requests at 64 B: MI355X_MICROARCH.md, HBM) + WRITE_SIZE [KB] x 1024
    (x 1.000 on a 1 GiB device copy: profiles/r1, r2).  Returns (traffic_bytes, source_text, sq_dict, binding_dict) — None for what
    could not be measured."""
    passes = {"FETCH_SIZE": ["FETCH_SIZE"], "WRITE_SIZE": ["WRITE_SIZE"],
              "SQ": ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_VMEM_RD", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_VALU", "GRBM_GUI_ACTIVE"],
              "TA": ["TA_BUSY_avr", "GRBM_GUI_ACTIVE"]}
    vals = _pmc_passes(passes, ["--kernel-only", "--no-group", "--steps", "3", "--warmup", "1", "--workload", wl.name, "--frames", str(B), "--feat-dtype", fdt,
                                "--path", str(path)] + (["--dev-lib"] if dev_lib else []),
                       lambda k: "cv_" in k and "_kernel" in k, timeout_s)
    traffic = src = sq = binding = None
    if "FETCH_SIZE" in vals and "WRITE_SIZE" in vals:
        traffic = float(f"{vals['FETCH_SIZE'] * 1024 * 2.0 + vals['WRITE_SIZE'] * 1024:.4g}")
        src = ("live: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over `bench.py --kernel-only` of this "
               "workload; FETCH_SIZE x 2.0 (gfx950 correction), WRITE_SIZE x 1.0; mean per launch")
    if "SQ_INSTS_VALU" in vals:
        iters = float(B * wl.h * wl.w * wl.V)                                    # (pixel, view) wave iterations per launch
        sq = {"valu_insts_per_pixel_view": round(vals["SQ_INSTS_VALU"] / iters, 2), "salu_insts_per_pixel_view": round(vals.get("SQ_INSTS_SALU", 0) / iters, 2),
              "vmem_insts_per_pixel_view": round(vals.get("SQ_INSTS_VMEM_RD", 0) / iters, 2), "lds_insts_per_pixel_view": round(vals.get("SQ_INSTS_LDS", 0) / iters, 2),
              "wave_cycles_waiting_frac": round(vals.get("SQ_WAIT_ANY", 0) / max(vals.get("SQ_WAVE_CYCLES", 1), 1), 3)}
    # which pipe the kernel actually occupies: GRBM_GUI_ACTIVE is summed over the 8 XCDs; SQ_ACTIVE_INST_VALU counts quad-cycles per SIMD
    # (x 4 / 1024 SIMDs); TA_BUSY_avr is the mean over the CUs' texture-address units
    g_sq, g_ta = vals.get("GRBM_GUI_ACTIVE"), vals.get("GRBM_GUI_ACTIVE@TA", vals.get("GRBM_GUI_ACTIVE"))
    if g_sq and "SQ_ACTIVE_INST_VALU" in vals:
        binding = {"valu_busy": round(vals["SQ_ACTIVE_INST_VALU"] * 4 / (1024 * g_sq / 8), 3),
                   "ta_busy": round(vals["TA_BUSY_avr"] / (g_ta / 8), 3) if "TA_BUSY_avr" in vals and g_ta else None,
                   "wait_frac": sq["wave_cycles_waiting_frac"] if sq else None,
                   "clock_ghz_in_kernel": round(g_sq / 8 / vals["_ns@SQ"], 3) if vals.get("_ns@SQ") else None,
                   "source": "live rocprofv3 --pmc passes over the kernel alone: vector-ALU busy share, address-unit (TA) busy share, share of wave "
                             "cycles spent waiting"}
    return traffic, src, sq, binding


def _step_child_args(a, steps, warmup):
    """The parent's own step configuration for a counter child: every flag that changes what a step executes is forwarded, so the
    counters describe the configuration of the line they are attached to; what is dropped are the flags that only add measurements
    (--full / --no-pmc / --no-cpu-baseline / --sustain-s are set by _pmc_passes) and the launcher's (--gpus).  --no-group: the child skips the
    process group (no RCCL initialisation and no weight broadcast inside the profiler's time budget)."""
    args = ["--steps", str(steps), "--warmup", str(warmup), "--workload", a.workload, "--no-group",
            "--path", str(a.path), "--conv-backend", a.conv_backend]
    if a.frames: args += ["--frames", str(a.frames)]
    if a.iters: args += ["--iters", str(a.iters)]
    if a.feat_dtype: args += ["--feat-dtype", a.feat_dtype]
    for flag, on in (("--no-fuse-tail", a.no_fuse_tail), ("--no-fuse-upsample", a.no_fuse_upsample), ("--no-graph", True),
                     ("--overlap", a.overlap), ("--overlap-pack", a.overlap_pack), ("--packed-inputs", a.packed_inputs),
                     ("--with-fnet", a.with_fnet), ("--dev-lib", a.dev_lib), ("--kernel-only", a.kernel_only), ("--nchw-out", a.nchw_out)):
        if on: args.append(flag)
    return args


def live_conv_counters(a, timeout_s=120):
    """Matrix-pipe busy share and in-kernel clock of the convolution launches, from one --pmc pass over a short child run of this
    same step — same flags as the parent (_step_child_args) — (SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs against GRBM_GUI_ACTIVE / 8 XCDs).
    None when the pass fails."""
    vals = _pmc_passes({"MFMA": ["SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE"]}, _step_child_args(a, 2, 1),
                       lambda k: "conv_mfma_kernel" in k, timeout_s)
    g = vals.get("GRBM_GUI_ACTIVE")
    if not g or "SQ_VALU_MFMA_BUSY_CYCLES" not in vals:
        return None
    return {"mfma_busy": round(vals["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024 / (g / 8), 3),
            "clock_ghz_in_kernel": round(g / 8 / vals["_ns@MFMA"], 3) if vals.get("_ns@MFMA") else None,
            "source": "live rocprofv3 --pmc pass over this step (same flags, no process group): mean over all conv_mfma_kernel dispatches"}


_RESULT_FD = None


def _claim_stdout():
    """The contract: rank 0's stdout carries ONE JSON line and nothing else.  Native libraries print to fd 1 behind Python's back (RCCL
    writes a five-line version banner to stdout when a process group is created): keep a private duplicate of the real stdout for the
    result line and point fd 1 at stderr for everything else.  Idempotent."""
    global _RESULT_FD
    if _RESULT_FD is None:
        sys.stdout.flush()
        _RESULT_FD = os.dup(1)
        os.dup2(2, 1)


def _emit_result(obj) -> None:
    line = (json.dumps(obj) + "\n").encode()
    if _RESULT_FD is None:
        sys.stdout.write(line.decode()); sys.stdout.flush()
    else:
        os.write(_RESULT_FD, line)


def _bound_label(binding, traffic, kern_ms):
    """What binds the fused kernel according to the live counters: "hbm" only if its measured HBM traffic runs at more than half of the
    peak rate; otherwise the busier of its two issue pipes, and "latency" when neither is above 85 % (waves waiting on dependent loads).
    Without counters the label is "unmeasured" — never an assumed "hbm"."""
    if traffic and kern_ms > 0 and traffic / (kern_ms * 1e-3) / 1e9 > 0.5 * HBM_PEAK_GBS:
        return "hbm"
    if not binding:
        return "unmeasured (no counter pass in this run)"
    v, t = binding.get("valu_busy") or 0.0, binding.get("ta_busy") or 0.0
    pipe = "vector-memory address unit (L1 gather)" if t >= v else "vector-ALU issue"
    return pipe if max(v, t) >= 0.85 else f"latency ({pipe} {max(v, t):.0%} busy, waves waiting {binding.get('wait_frac')})"


def spawn_ranks(n: int, poll_s: float = 0.2, grace_s: float = 5.0) -> int:
    """Re-run this command line as n processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment, one GPU
    each via LOCAL_RANK -> torch.cuda.set_device), as the reference spawns its DDP workers (train_MaGNet.py:323-338).
    Rank 0's stdout (the JSON line) passes through; every rank's stderr passes through tagged "[rank r]"; the stdout of
    ranks > 0 is forwarded to stderr with the same tag.  ALL children are polled: the first one that exits non-zero (or is
    killed) takes the others down (SIGTERM, SIGKILL after `grace_s`) — a dead rank must not leave the rest waiting in an
    RCCL barrier until the collective timeout — and its return code is this launcher's."""
    import socket
    import subprocess
    import threading
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    procs, pumps = [], []

    def pump(stream, tag):
        for line in iter(stream.readline, ""):
            sys.stderr.write(f"{tag} {line}" if line.strip() else line)
        stream.close()

    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        pr = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, text=True, bufsize=1,
                              stdout=None if r == 0 else subprocess.PIPE, stderr=subprocess.PIPE)
        procs.append(pr)
        for st in ([pr.stderr] if r == 0 else [pr.stderr, pr.stdout]):
            t = threading.Thread(target=pump, args=(st, f"[rank {r}]"), daemon=True); t.start(); pumps.append(t)
    rc, alive = 0, set(range(n))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 128 - code                  # killed by signal s -> 128 + s
                sys.stderr.write(f"[bench launcher] rank {r} exited with {code}: stopping the other {len(alive)} rank(s)\n")
                for o in alive:
                    procs[o].terminate()
                t_end = time.monotonic() + grace_s
                while time.monotonic() < t_end and any(procs[o].poll() is None for o in alive):
                    time.sleep(poll_s)
                for o in alive:
                    if procs[o].poll() is None:
                        procs[o].kill()
        if alive:
            time.sleep(poll_s)
    for t in pumps:
        t.join(timeout=2.0)
    return rc


def dry_run(a, rank, world):
    """Everything around the kernels, on CPU tensors with gloo: rendezvous, the one flat weight broadcast, frame sharding,
    barrier + max-over-ranks timing, the JSON line.  No HIP call is made (and none is reported: value is null)."""
    from magnet_amd.magnet import GNET
    wl = synth.WORKLOADS[a.workload]
    torch.manual_seed(1234 + rank)
    net = GNET(ch_in=256 + wl.D)
    bcast_bytes = mdist.broadcast_module_(net, src=0)
    bcast_ok = mdist.broadcast_verified(net) if bcast_bytes else None
    fnet_bytes = 0
    if a.with_fnet:                                          # the shared F-Net weights north_star names: their own flat bucket(s)
        from types import SimpleNamespace
        from magnet_amd import fnet as mfnet
        fnet = mfnet.FNET(SimpleNamespace(FNET_architecture="PSM-Net", FNET_feature_dim=wl.F))
        fnet_bytes = mdist.broadcast_module_(fnet, src=0)
        bcast_ok = bool(bcast_ok) and mdist.broadcast_verified(fnet)
    local = int(os.environ.get("LOCAL_RANK", rank))
    cpus = mdist.pin_to_cpu_slice(local, int(os.environ.get("LOCAL_WORLD_SIZE", 0)) or world)
    n_cpus = mdist.gather_floats(float(len(cpus)))
    B = a.frames or 4
    lo, hi = mdist.shard_range(world * B, rank, world)
    mdist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        pass
    mdist.barrier()
    mine = time.perf_counter() - t0
    elapsed = mdist.max_over_ranks(mine)
    per_rank = mdist.gather_floats((hi - lo) * a.steps / max(mine, 1e-9))
    frames = mdist.sum_over_ranks(hi - lo)
    if rank == 0:
        _emit_result({"metric": "dry-run (launcher self-test, no kernels)", "value": None, "unit": "ref-frames/s",
                          "per_rank_frames_per_s": per_rank,
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / max(1, a.steps),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": wl.name, "frames_per_step_all_ranks": int(frames),
                                     "parallelism": f"frames sharded over {world} rank(s); one weight broadcast ({bcast_bytes} B)"},
                          "weight_broadcast_bytes": bcast_bytes, "fnet_weight_broadcast_bytes": fnet_bytes,
                          "rccl": {"world": world, "backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else None,
                                   "broadcast_bytes": bcast_bytes + fnet_bytes, "broadcast_verified": bcast_ok},
                          "cpus_per_rank": [int(v) for v in n_cpus],
                          **({"counters": "N=1 only", "cpu_baseline": "N=1 only"} if world > 1 else {})})
    mdist.barrier()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="C2", choices=sorted(synth.WORKLOADS))
    ap.add_argument("--frames", type=int, default=0, help="reference frames per GPU per step (0 = auto)")
    ap.add_argument("--iters", type=int, default=0, help="refinement iterations (0 = workload default)")
    ap.add_argument("--feat-dtype", default="", choices=["", "fp32", "bf16"])
    ap.add_argument("--path", type=int, default=0, help="matcher kernel (include/magnet_hip.h): 0 production, 1 generic exact, 2 exact candidate-lane, 3 worklist")
    ap.add_argument("--conv-backend", default="mfma", choices=["mfma", "torch"],
                    help="g_net/mask_head convolutions: bf16x3 MFMA kernel (default) or nn.Conv2d on MIOpen")
    ap.add_argument("--no-fuse-tail", action="store_true", help="one launch per 1x1 layer instead of the fused epilogue")
    ap.add_argument("--no-fuse-upsample", action="store_true", help="mask head writes its (B,144,h,w) logits and a separate launch upsamples "
                    "(default: the mask head's last layer writes the upsampled predictions itself)")
    ap.add_argument("--graph", action="store_true", help="(default since round 6) replay the step as one HIP graph (magnet_amd/graph.py)")
    ap.add_argument("--no-graph", action="store_true", help="launch the step's kernels eagerly from the host instead of replaying a captured HIP graph")
    ap.add_argument("--overlap", action="store_true", help="run the mask head on a side stream (measured: no gain)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="step = the fused cost-volume kernel alone")
    ap.add_argument("--nchw-out", action="store_true", help="--kernel-only: write the reference's (B,D,h,w) fp32 volume instead of the "
                    "split-bf16 channel-last form the step uses (the G-Net input buffer)")
    ap.add_argument("--no-pmc", action="store_true", help="skip the live rocprofv3 counter passes (roofline.traffic = null)")
    ap.add_argument("--packed-inputs", action="store_true", help="backbone outputs arrive in the kernels' layouts (features "
                    "channel-last as the matrix-core F-Net writes them, x_d3 in the G-Net input buffer): no pack pass in the step")
    ap.add_argument("--overlap-pack", action="store_true", help="x_d3 repack on a side stream beside the matcher (measured: no gain)")
    ap.add_argument("--sustain-s", type=float, default=6.0, help="extra untimed-by-contract run of this many seconds after the K "
                    "steps, reported as sustained_frames_per_s (--full only; 0 = skip)")
    ap.add_argument("--with-fnet", action="store_true", help="the step starts from the IMAGES: F-Net (matrix-core path, magnet_amd/fnet.py) on the "
                    "1 + V images of every reference frame, then the loop; D-Net outputs stay resident synthetic tensors (torch.hub "
                    "backbone, not buildable offline).  Reported beside the contract line, never instead of it")
    ap.add_argument("--dev-lib", action="store_true", help="tools/ only: bind to libmagnet_hip_dev.so (python -m magnet_amd.build --dev), "
                    "the build that honours the MAGNET_* variant switches; never a valid result line")
    ap.add_argument("--no-group", action="store_true", help="no process group for a plain one-process launch (what bench.py's own rocprofv3 "
                    "counter children use); ignored under a launcher (RANK set)")
    ap.add_argument("--dry-run", action="store_true", help="launcher / distributed self-test without a GPU: gloo backend, "
                    "the step is a no-op (used by tests/test_bench_launcher.py)")
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure roofline / roofline_conv (HIP-event pass, "
                    "rocprofv3 counter passes), the sustained rate, the packed-input step and the CPU baseline, and at N=1 create the "
                    "one-rank process group with the verified weight broadcast; a plain run times the steps and nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="after the timed steps write what the last one returned as "
                    "DIR/<name>.npy (float32; a fixed seeded sample when it exceeds 60 MB)")
    a = ap.parse_args()
    if a.steps < 1 and not a.dry_run:
        ap.error("--steps must be at least 1")

    if a.gpus > 1 and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves, one process per GPU (the reference spawns its
        # DDP workers the same way, train_MaGNet.py:323-338); under torch.distributed.run the environment is already set
        raise SystemExit(spawn_ranks(a.gpus))

    _claim_stdout()
    if os.environ.get("MAGNET_BENCH_FAIL_RANK") == os.environ.get("RANK", "0") and a.dry_run:
        raise SystemExit(3)                                  # launcher self-test (tests/test_bench_launcher.py): this rank dies early
    rccl = {"world": 1, "backend": None, "broadcast_bytes": 0, "broadcast_verified": None}
    try:
        # --full: a process group on a GPU — one rank included: RCCL initialisation and the weight broadcast run under the N = 1 clock
        # exactly as they will at N = 8 (train_MaGNet.py:197-210).  A plain N = 1 run needs no collective for its headline
        rank, world, local = mdist.init_from_env(backend="gloo" if a.dry_run else None,
                                                 always=(a.dry_run or (a.full and torch.cuda.is_available())) and not a.no_group)
    except Exception as e:                                   # a one-rank RCCL group that cannot be created must not take the N = 1 line down
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise
        print(f"[bench] process-group initialisation failed ({type(e).__name__}: {e}); continuing single-process", file=sys.stderr)
        rccl["error"] = f"{type(e).__name__}: {e}"[:200]
        rank, world, local = 0, 1, 0
    if world != a.gpus and rank == 0:
        print(f"[bench] note: --gpus {a.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    if a.dry_run:
        return dry_run(a, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    from magnet_amd import build as mbuild, lib
    if a.dev_lib:
        lib.use_dev_build()
    if rank == 0:
        mbuild.build(dev=a.dev_lib)                           # (a stale library is recompiled on all of the node's CPUs: pin afterwards)
    mdist.barrier()
    lib.load()
    # one node: a contiguous CPU slice per LOCAL rank (MAGNET_BENCH_AFFINITY=0: off)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", 0)) or min(world, max(1, torch.cuda.device_count()))
    cpus = mdist.pin_to_cpu_slice(local, local_world)
    from magnet_amd.homography import CostVolumeCW
    from magnet_amd.magnet import MAGNET

    wl = synth.WORKLOADS[a.workload]
    iters = a.iters or wl.iters
    fdt = a.feat_dtype or wl.feat_dtype
    # enough frames per step that one launch fills the chip and the working set exceeds the 256 MiB L3
    B = a.frames or max(1, min(16 if a.with_fnet else 64, int(round(1200e6 / max(wl.algorithmic_bytes(), 1)))))
    torch.manual_seed(1234)                               # every rank draws its own init; rank 0's wins below
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=r"MAGNET. args\.\w+_ckpt is not set")   # no backbones here: the bench starts from their outputs
        model = MAGNET(make_args(wl, iters), d_net=_NoBackbone(), f_net=_NoBackbone(), feat_dtype=fdt,
                       conv_backend=a.conv_backend)
    model_cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        import copy
        model_cpu = copy.deepcopy(model).eval()
    model = model.to(device).eval()
    model.overlap_mask_head = a.overlap
    model.overlap_pack = a.overlap_pack
    model.fuse_conv_tail = not a.no_fuse_tail
    model.fuse_upsample = not a.no_fuse_upsample
    bcast_bytes = mdist.broadcast_module_(model, src=0)   # the one RCCL collective (weights), xGMI
    bcast_ok = mdist.broadcast_verified(model, device=device) if bcast_bytes and a.full else None

    # north_star: "RCCL-over-xGMI broadcast of shared F-Net weights": the 13.4 MB bucket travels in the --full line too (the F-Net itself
    # runs inside the step only with --with-fnet)
    fnet_bcast_bytes = 0
    if a.full and torch.distributed.is_available() and torch.distributed.is_initialized() and not a.with_fnet and not a.kernel_only:
        from magnet_amd import fnet as mfnet_b
        fa_b = make_args(wl, iters); fa_b.FNET_architecture = "PSM-Net"
        fnet_b = mfnet_b.FNET(fa_b).to(device).eval()
        fnet_bcast_bytes = mdist.broadcast_module_(fnet_b, src=0)
        bcast_ok = bool(bcast_ok) and mdist.broadcast_verified(fnet_b, device=device)
        del fnet_b
    inp = device_inputs(wl, B, seed=1000 + rank, device=device)
    k_list = model.k_list
    ev_pairs = []
    conv_events = []
    from magnet_amd.convnet import ConvStackMFMA

    model.matcher_path = a.path
    graph_state = "eager"
    if a.with_fnet:
        from magnet_amd import fnet as mfnet

        class _ResidentDNet(torch.nn.Module):                # D-Net outputs ((mu, sigma) maps, x_d3) as resident tensors
            def __init__(self, gmms, x_d3):
                super().__init__(); self.gmms, self.x_d3 = gmms, x_d3

            def forward(self, img):
                return self.gmms, self.x_d3
        fa = make_args(wl, iters); fa.FNET_architecture = "PSM-Net"
        model.f_net = mfnet.FNET(fa).to(device).eval()
        fnet_bcast_bytes = mdist.broadcast_module_(model.f_net, src=0)   # the shared F-Net weights (13.4 MB): their own flat bucket(s)
        if fnet_bcast_bytes and a.full:
            bcast_ok = bool(bcast_ok) and mdist.broadcast_verified(model.f_net, device=device)
        model.d_net = _ResidentDNet(torch.cat([inp["ref_gmms"], inp["nghbr_gmms"]], dim=0),
                                    inp["x_d3"])          # the forward keeps x_d3[:B] only (MAGNET.py:139)
        model.fnet_mfma = True
        gi = torch.Generator(device=device).manual_seed(77 + rank)
        ref_img = torch.randn(B, 3, 4 * wl.h, 4 * wl.w, generator=gi, device=device)
        nb_img = torch.randn(wl.V * B, 3, 4 * wl.h, 4 * wl.w, generator=gi, device=device)

        def step(timed):
            CostVolumeCW.event_sink = ev_pairs if timed else None
            ConvStackMFMA.event_sink = conv_events if timed else None
            with torch.no_grad():
                return model(ref_img, nb_img, inp["nghbr_poses"], inp["is_valid"], inp["cam_intrins"], mode="test")
    elif a.kernel_only:
        matcher = CostVolumeCW(inp["ref_feat"], inp["nghbr_feat"], inp["nghbr_gmms"], inp["nghbr_poses"],
                               inp["is_valid"], inp["cam_intrins"], 5, feat_dtype=fdt, path=a.path)
        if a.nchw_out:
            kw = dict(out=torch.empty(B, wl.D, wl.h, wl.w, device=device))
            kernel_out = {"cost": kw["out"]}
        else:                                               # the form the step uses: the D cost channels of the G-Net input buffer
            ld = (wl.D + 7) // 8 * 8 + 256
            hi = torch.zeros(B * (wl.h + 2) * (wl.w + 2), ld, dtype=torch.bfloat16, device=device)
            kw = dict(out_split=(hi, torch.zeros_like(hi), ld))
            kernel_out = {"cost_hi": hi[:, :wl.D], "cost_lo": kw["out_split"][1][:, :wl.D]}

        def step(timed):
            CostVolumeCW.event_sink = ev_pairs if timed else None   # HIP events around the fused kernel
            matcher(ref_gmm=inp["ref_gmms"], k_list=k_list, **kw)
            return kernel_out
    elif a.packed_inputs:
        # what a backbone on the matrix-core path hands over: features in the matcher's layouts (magnet_amd/fnet.py writes
        # exactly these), x_d3 already in the G-Net input buffer.  Packed ONCE, outside the timed region.
        packed = (lib.pack_features(inp["ref_feat"], lib.feat_enum(fdt), pad=0), lib.pack_features(inp["nghbr_feat"], lib.feat_enum(fdt), pad=1))
        gh, gl, ctot, coff = model.gnet_input_buffer(B, wl.h, wl.w, device)
        lib.pack_split(inp["x_d3"], gh, gl, ctot, coff)

        def step(timed):
            CostVolumeCW.event_sink = ev_pairs if timed else None
            ConvStackMFMA.event_sink = conv_events if timed else None
            with torch.no_grad():
                return model.match_and_refine(inp["ref_gmms"], None, None, None, inp["nghbr_gmms"], inp["nghbr_poses"], inp["is_valid"],
                                              inp["cam_intrins"], mode="test", packed_feats=packed, x_d3_in_place=True)
    else:
        def eager_step(timed):
            CostVolumeCW.event_sink = ev_pairs if timed else None
            ConvStackMFMA.event_sink = conv_events if timed else None
            with torch.no_grad():
                return model.match_and_refine(inp["ref_gmms"], inp["x_d3"], inp["ref_feat"], inp["nghbr_feat"],
                                              inp["nghbr_gmms"], inp["nghbr_poses"], inp["is_valid"],
                                              inp["cam_intrins"], mode="test")
        step = eager_step
        if not a.no_graph and a.conv_backend == "mfma":
            # The step as ONE captured HIP graph (magnet_amd/graph.py): the same launches in the same order on the same resident inputs,
            # replayed without the host in the loop (5.78 -> 5.69 ms per C2 step, same box).  The instrumented pass below (HIP events around
            # the matcher / convolution launches) runs the eager form: events cannot be read out of a replay, the kernels are the same.
            # A capture that fails for any reason leaves the eager step in place and says so in the line.
            try:
                from magnet_amd.graph import GraphedRefine
                graphed = GraphedRefine(model, inp["ref_gmms"], inp["x_d3"], inp["ref_feat"], inp["nghbr_feat"], inp["nghbr_gmms"],
                                        inp["nghbr_poses"], inp["is_valid"], inp["cam_intrins"], mode="test")

                def step(timed):
                    if timed:
                        return eager_step(True)
                    return graphed(*graphed.static)         # inputs already in place: replay only; the graph's static outputs
                graph_state = "replay"
            except Exception as e:                          # noqa: BLE001 — any capture failure: measure the eager step
                print(f"[bench] HIP-graph capture failed ({type(e).__name__}: {e}); timing the eager step", file=sys.stderr)
                graph_state = f"capture failed ({type(e).__name__}): eager"
                step = eager_step

    for _ in range(a.warmup):
        step(False)
    torch.cuda.synchronize(); mdist.barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step(False)                                    # the contract's timed region holds the step and nothing else
    torch.cuda.synchronize()
    mine = time.perf_counter() - t0                          # this rank's own time for its K steps (before the closing barrier)
    mdist.barrier(); torch.cuda.synchronize()
    elapsed = mdist.max_over_ranks(time.perf_counter() - t0, device=device)
    per_rank = mdist.gather_floats(B * a.steps / max(mine, 1e-9), device=device)   # a straggler GPU shows here, not only in the max
    if a.dump_outputs and rank == 0:                         # before anything else runs the step (a replay overwrites its outputs)
        names = dump_outputs(out, a.dump_outputs)
        print(f"[bench] last timed step's outputs written to {a.dump_outputs}: {', '.join(names)}", file=sys.stderr)

    # kernel times (roofline / roofline_conv): the same K steps again, back to back with the timed region, with HIP events on
    # the launch stream around the matcher and the convolution launches (kept out of the contract's clock: ~6 events per step)
    if a.full:
        for _ in range(a.steps):
            step(True)
        torch.cuda.synchronize()
        CostVolumeCW.event_sink = None; ConvStackMFMA.event_sink = None

    # steady state: the contract's K steps take ~0.2 s, before the chip has settled at its sustained clock under continuous
    # matrix-core load; run on for --sustain-s seconds (outside the contract's timed region) and report that rate too
    sustained = None
    if a.full and a.sustain_s > 0:
        n_sus, t_s = 0, time.perf_counter()
        while True:
            for _ in range(10):
                step(False)
            n_sus += 10
            torch.cuda.synchronize()
            if time.perf_counter() - t_s >= a.sustain_s:
                break
        mdist.barrier()
        sus_elapsed = mdist.max_over_ranks(time.perf_counter() - t_s, device=device)
        sustained = world * B * n_sus / sus_elapsed

    # the same step when the backbones hand their outputs over in the kernels' layouts (what magnet_amd/fnet.py's F-Net does):
    # no pack pass.  Reported next to the contract number, never instead of it.
    packed_ms = None
    if a.full and not (a.kernel_only or a.packed_inputs or a.with_fnet) and a.conv_backend == "mfma":
        packed = (lib.pack_features(inp["ref_feat"], lib.feat_enum(fdt), pad=0), lib.pack_features(inp["nghbr_feat"], lib.feat_enum(fdt), pad=1))
        gh, gl, ctot, coff = model.gnet_input_buffer(B, wl.h, wl.w, device)
        lib.pack_split(inp["x_d3"], gh, gl, ctot, coff)
        CostVolumeCW.event_sink = None; ConvStackMFMA.event_sink = None

        def pstep():
            with torch.no_grad():
                model.match_and_refine(inp["ref_gmms"], None, None, None, inp["nghbr_gmms"], inp["nghbr_poses"], inp["is_valid"],
                                       inp["cam_intrins"], mode="test", packed_feats=packed, x_d3_in_place=True)
        for _ in range(3):
            pstep()
        torch.cuda.synchronize(); t_p = time.perf_counter()
        for _ in range(a.steps):
            pstep()
        torch.cuda.synchronize()
        packed_ms = mdist.max_over_ranks(1e3 * (time.perf_counter() - t_p) / a.steps, device=device)

    kern_ms = sum(e0.elapsed_time(e1) for e0, e1 in ev_pairs) / max(1, len(ev_pairs))
    # HBM traffic and instruction counters of the fused kernel: measured LIVE by separate rocprofv3 --pmc passes over a
    # kernel-only child run of this same workload (rank 0, one GPU, production path only; null when the profiler is not
    # available or a pass fails — never a stored number)
    traffic, traffic_src, pmc, binding, conv_binding = None, None, None, None, None
    if a.full and rank == 0 and world == 1 and not a.no_pmc and not a.kernel_only and a.path == 0:
        traffic, traffic_src, pmc, binding = live_counters(wl, B, fdt, path=a.path, dev_lib=a.dev_lib)
        if a.conv_backend == "mfma" and not a.with_fnet:
            conv_binding = live_conv_counters(a)
    alg_bytes = wl.algorithmic_bytes() * B
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9 if kern_ms > 0 else 0.0
    frames = world * B * a.steps
    # the 3x3 convolution launches (9 taps): the dominant kernel of the step by time
    c3 = [(e0.elapsed_time(e1), fl) for e0, e1, fl, taps in conv_events if taps == 9]
    conv_ms_all = sum(e0.elapsed_time(e1) for e0, e1, _, _ in conv_events) / max(1, a.steps)

    if rank == 0:
        grid_desc = (f"{wl.h}x{wl.w} matching grid (grid-stress variant)" if wl.name.endswith(("L", "Lf"))
                     else f"{4 * wl.h}x{4 * wl.w} input -> {wl.h}x{wl.w} matching grid")
        workload_desc = (f"{wl.name}: {wl.camera} {grid_desc}, V={wl.V} source views, D={wl.D} candidates, "
                         f"F={wl.F}, I={iters} iteration(s), {fdt} feature storage")
        res = {
            "metric": "ref-frames/sec (640x480, 4 src, 64 cand) + warp-kernel HBM GB/s",
            "value": frames / elapsed, "unit": "ref-frames/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": 1e3 * elapsed / a.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": workload_desc,
                       "feature_storage": fdt, "arithmetic": "fp32 (matcher: fp32 view accumulation, tolerance-parity geometry; convolutions "
                                                             "bf16x3-split on the matrix cores with fp32 accumulation)",
                       "inputs": (f"{1 + wl.V} images of {4 * wl.h}x{4 * wl.w} per reference frame; F-Net (PSMNet, matrix-core path) INSIDE the step, D-Net "
                                  "outputs resident" if a.with_fnet else
                                  "backbone outputs in the kernels' layouts (no pack pass)" if a.packed_inputs else
                                  "backbone outputs as the reference's NCHW fp32 tensors (pack passes inside the step)"),
                       "frames_per_gpu_per_step": B, "step": "kernel-only" if a.kernel_only else
                       ("F-Net on every image + " if a.with_fnet else "") +
                       ("pack + I x (fused cost volume + G-Net + Gaussian update) + mask head with the convex upsampling in its last layer; convs on "
                        + ("the bf16x3 MFMA kernel" if a.conv_backend == "mfma" else "MIOpen fp32")
                        + ("; the step's launches replayed as one captured HIP graph" if graph_state == "replay" else "; launched eagerly from the host")),
                       "launch": graph_state,
                       "parallelism": f"frames sharded over {world} GPU(s), no data-path collective; "
                                      + (f"one RCCL weight broadcast ({bcast_bytes} B)" if bcast_bytes else "no process group")},
            "weight_broadcast_bytes": bcast_bytes, "fnet_weight_broadcast_bytes": fnet_bcast_bytes,
            "rccl": dict(rccl, world=world, backend=(torch.distributed.get_backend() if torch.distributed.is_available() and torch.distributed.is_initialized() else None),
                         broadcast_bytes=bcast_bytes + fnet_bcast_bytes, broadcast_verified=bcast_ok),
            "cpus_per_rank": len(cpus),
            "per_rank_frames_per_s": per_rank,
            "per_rank_min_max": [min(per_rank), max(per_rank)],
        }
        if a.full:
            res.update({
                # `frac` is against the HBM roofline (the contract's target); `bound` says what the counters say binds the kernel
                "roofline": {"bound": _bound_label(binding, traffic, kern_ms), "contract_roofline": "hbm",
                             "kernel": "fused sample+warp+score (magnet_cost_volume_cw)",
                             "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                             "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": kern_ms,
                             "launches_timed": len(ev_pairs)},
                "cost_volume_frames_per_s": B / (kern_ms * 1e-3) if kern_ms > 0 else None,
                "sustained_frames_per_s": sustained,
                "ms_per_step_inputs_in_kernel_layouts": packed_ms,
                "frames_per_s_inputs_in_kernel_layouts": (world * B / (packed_ms * 1e-3)) if packed_ms else None,
            })
            if pmc:
                res["roofline"]["sq_counters"] = pmc            # instructions per (pixel, view), wait fraction: measured in this run
            if binding:
                res["roofline"]["binding"] = binding
            if c3:
                t3 = sum(t for t, _ in c3) / len(c3); f3 = sum(f for _, f in c3) / len(c3)
                res["roofline_conv"] = {
                    "bound": "mfma", "kernel": "3x3 implicit-GEMM convolution (magnet_conv_mfma, bf16x3 split operands)",
                    "achieved": f3 / (t3 * 1e-3) / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                    "frac": f3 / (t3 * 1e-3) / 1e12 / 2500.0,
                    "note": "achieved = algorithmic fp32-equivalent flops (2*M*N*K) per launch / HIP-event time; the kernel "
                            "executes 3 bf16 MFMAs per product term, so matrix-pipe utilisation is 3x this fraction",
                    "algorithmic_flops_per_launch": f3, "avg_launch_ms": t3, "launches_timed": len(c3),
                    "all_conv_layers_ms_per_step": conv_ms_all}
                if conv_binding:
                    res["roofline_conv"].update(conv_binding)
            if model_cpu is not None:
                res["cpu_baseline"] = cpu_baseline(wl, model_cpu, iters)
            if world > 1:
                # the contract: counters (roofline.traffic / binding, roofline_conv.mfma_busy) and the CPU baseline are measured on rank 0 of
                # the N = 1 run only; say so in the N > 1 line instead of leaving the fields silently absent
                res["roofline"]["traffic_source"] = "N=1 only (live rocprofv3 passes run in the one-GPU launch)"
                res["counters"] = "N=1 only"
                res["cpu_baseline"] = "N=1 only"
        _emit_result(res)
    mdist.barrier()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
