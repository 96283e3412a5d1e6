"""HIP-graph replay of the refinement loop: the host leaves the loop.

At 64 frames per step the path is GPU-bound (5.8 ms of kernels, ~15 device operations): replaying the captured step still saves the
inter-operation gaps — 5.78 -> 5.69 ms per C2 step (11 067 -> 11 239 frames/s), same box (profiles/r6/graph_replay_ab.jsonl; bench.py
replays the step this way by default, --no-graph: eager).  The reference's own evaluation loop feeds ONE frame at a time
(test_MaGNet.py:166-170, batch size 1).  `GraphedRefine` captures `MAGNET.match_and_refine` for a fixed shape into a HIP graph once
(torch.cuda.CUDAGraph: our kernels are launched on torch's capture stream, so they are recorded like torch's own) and replays it per
frame: one launch from the host's point of view.  At one frame the host is what an eager step waits for: the shipped step (D = 5,
I = 3) takes 0.5365 ms launched eagerly and 0.3001 ms replayed, the C2 step 0.3640 and 0.1910 ms (bench.py --frames 1, medians of six
fresh processes: profiles/latency/bench_frames1.jsonl).  What remains is the serial chain of ~13 kernels that each under-fill the chip
(one frame = 152 convolution tiles of 128 rows for 256 CUs; on 64-row tiles, ConvStackMFMA.small_tiles = True, the replayed shipped
step takes 0.2938 against 0.2986 ms and the C2 step 0.1882 against 0.1874 ms, not a gain in every pair at every workload, so it is opt-in:
profiles/latency/NOTES.md) — batching frames is what pays.  Inputs are copied into the graph's static tensors (device-to-device,
a few MB); outputs are the graph's static output tensors (clone them to keep a result across replays).

`GraphedRefine` covers `match_and_refine` on NCHW tensors alone.  A stream of frames, with the backbones, the frame pool's gather and
the packed / in-place forms inside the replayed step, is `magnet_amd.sequence.SequenceRunner(model, capacity, graph=True)`."""
from __future__ import annotations

import torch

from . import lib


class GraphedRefine:
    def __init__(self, model, ref_gmms, x_d3, ref_feat, nghbr_feat, nghbr_gmms, nghbr_poses, is_valid, cam_intrins, mode="test",
                 warmup: int = 3):
        if not ref_feat.is_cuda:
            raise lib.MagnetError("GraphedRefine: tensors must be on the GPU (no CPU fallback)")
        dev = ref_feat.device
        self.model, self.mode = model, mode
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        self.static = [f32(t) for t in (ref_gmms, x_d3, ref_feat, nghbr_feat, nghbr_gmms, nghbr_poses)]
        # validity and intrinsics live in static device tensors too, so they can change between replays
        self.is_valid = is_valid.detach().to(device=dev, dtype=torch.int32).contiguous().clone()
        self.cam = {k: v.detach().to(device=dev, dtype=torch.float32).contiguous().clone() for k, v in cam_intrins.items()}
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():                  # warm-up outside capture: workspaces, weight packs, attributes
            for _ in range(max(1, warmup)):
                model.match_and_refine(*self.static, self.is_valid, self.cam, mode=mode)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # thread-local capture mode: another thread of the process that polls events meanwhile (torch.distributed's RCCL watchdog, once
        # a process group exists — bench.py always has one) must not invalidate this thread's capture
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"), torch.no_grad():
            self.out = model.match_and_refine(*self.static, self.is_valid, self.cam, mode=mode)

    def __call__(self, ref_gmms, x_d3, ref_feat, nghbr_feat, nghbr_gmms, nghbr_poses, is_valid=None, cam_intrins=None):
        for s, t in zip(self.static, (ref_gmms, x_d3, ref_feat, nghbr_feat, nghbr_gmms, nghbr_poses)):
            if t is not s:
                s.copy_(t, non_blocking=True)
        if is_valid is not None:
            self.is_valid.copy_(is_valid.to(torch.int32), non_blocking=True)
        if cam_intrins is not None:
            for k in self.cam:
                self.cam[k].copy_(cam_intrins[k], non_blocking=True)
        self.graph.replay()
        return self.out
