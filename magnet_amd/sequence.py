"""Sequence inference: run each frame's backbones once, gather views.

`MAGNET.forward` runs the D-Net and the F-Net on all B (1 + V) images of every call, as the reference does.  On a video, or on a
scene walked with `data.window_indices`, the same frame is a neighbour of several windows and the reference of one, and its F-Net
features, its D-Net (mu, sigma) and its x_feat depend on that image alone.  `FramePool` keeps them on the device, one slot per
frame, in the layouts the kernels read; `SequenceRunner` encodes the frames a call has not seen, and one `lib.gather_views`
launch (csrc/frame_pool.hip) assembles the matcher's and G-Net's inputs of a step from the pool through a device table of slots.

    runner = SequenceRunner(model, capacity=64)
    pred_list = runner.forward(ref_ids, ref_img, nghbr_ids, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, mode="test")

Frame ids are any hashable, e.g. (scene_name, img_idx); None stands for "no frame" (zeros; the view must be off in is_valid).
Ids and slots are host objects, tensors stay on the device: nothing here waits for the device.  Inference only.

Streaming (`SequenceRunner(model, capacity, graph=True)`, opt-in): one new frame per step, B = 1, is bound by the host — about a
hundred launches that each under-fill the chip.  In graph mode add() and refine() replay captured HIP graphs.  What makes a step
replayable is that no launch argument depends on the slots the host picked: the backbones always write to staging buffers,
one `lib.scatter_frames` launch (magnet_scatter_frames, the gather's inverse) moves them into the pool through a device table, and
the tables reach the device through a small ring of pinned rows.  See SequenceRunner for what a graph holds and when it is
captured again; tools/bench_stream.py and profiles/stream/NOTES.md for what it buys.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import lib
from .lib import MagnetError


def _first_missing(frame_ids, held):
    """Positions in `frame_ids` of the first occurrence of every id that is not in `held` (None is no frame)."""
    seen, out = set(), []
    for i, fid in enumerate(frame_ids):
        if fid is not None and fid not in held and fid not in seen:
            seen.add(fid)
            out.append(i)
    return out


def _runs(values):
    """[(position, value, length)] of the maximal runs of consecutive integers in `values`."""
    out = []
    for i, v in enumerate(values):
        if out and out[-1][1] + out[-1][2] == v:
            out[-1] = (out[-1][0], out[-1][1], out[-1][2] + 1)
        else:
            out.append((i, v, 1))
    return out


def _tensors(obj, out=None):
    """Every tensor reachable from `obj` through dicts, lists and tuples, in a fixed order."""
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, dict):
        for k in obj:
            _tensors(obj[k], out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors(v, out)
    return out


def _weights_key(modules):
    """(data_ptr, _version) of every parameter and buffer under `modules`: what planes.PackCache keys a weight pack on (an optimiser
    step, load_state_dict or a BatchNorm update bumps _version, a replaced tensor has another address), read from the modules' own
    dicts, which is several times cheaper than Module.parameters() + buffers()."""
    return tuple((t.data_ptr(), t._version) for top in modules for m in top.modules()
                 for d in (m._parameters, m._buffers) for t in d.values() if t is not None)


class _TableRing:
    """A slot table's way to the device: `rows` pinned host rows used in turn, each with an event recorded behind its copy.  A row
    is written again only `rows` steps later; its event is waited for then (long complete, unless the host runs that far ahead)."""

    def __init__(self, width, device, rows=8):
        self.host = torch.zeros((rows, width), dtype=torch.int32).pin_memory()
        self.dev = torch.zeros((width,), dtype=torch.int32, device=device)
        self.events = [None] * rows
        self.next = 0

    def push(self, values):
        r, self.next = self.next, (self.next + 1) % len(self.events)
        if self.events[r] is None:
            self.events[r] = torch.cuda.Event()
        else:
            self.events[r].synchronize()                 # the ring has wrapped: the copy that read this row must be over
        self.host[r].copy_(torch.tensor(values, dtype=torch.int32))
        self.dev.copy_(self.host[r], non_blocking=True)
        self.events[r].record(torch.cuda.current_stream(self.dev.device))


class _Static:
    """A device tensor a captured graph reads, refilled before a replay.  A host tensor is uploaded only when its content differs from
    the last upload (is_valid and the intrinsics of a stream rarely change; a pageable upload would wait for the device)."""

    def __init__(self, t, device, dtype=None):
        self.t = t.detach().to(device=device, dtype=dtype or t.dtype).contiguous().clone()
        self.sig = (tuple(self.t.shape), self.t.dtype)
        self._host = self._host_key(t)

    @staticmethod
    def _host_key(t):
        if t.is_cuda:
            return None
        t = t.detach().contiguous()
        if t.numel() * t.element_size() <= (1 << 20):
            return (str(t.dtype), t.numpy().tobytes())
        return (str(t.dtype), t.data_ptr(), t._version)

    def load(self, t):
        if t is self.t:
            return
        key = self._host_key(t)
        if key is not None and key == self._host:
            return
        self._host = key
        self.t.copy_(t.detach(), non_blocking=True)


class _Captured:
    """The captured HIP graphs of one SequenceRunner step: one or more parts, replayed in order.  Subclasses give `parts()`:
    [(launch, watched)], where launch() issues the part's launches on the current stream (reading the statics, returning its outputs)
    and watched() names what those launches bake in: the caches whose tensors' addresses they use, the weight caches, and the
    modules whose weights those were packed from.  A part keeps a reference to every such tensor, so none of them can be freed (and
    its address handed out again) while the graph lives, and a fingerprint: their addresses and the weights' (data_ptr, _version).
    replay() recomputes a part's fingerprint (host arithmetic only) right before it replays that part, so the check of part i + 1
    runs while the device works on part i."""

    def __init__(self, runner, key):
        self.runner, self.key = runner, key
        self.graphs, self.outs, self.keep, self.fps = [], [], [], []
        self._parts = None

    @property
    def out(self):
        return self.outs[-1]

    @staticmethod
    def _fingerprint(watched):
        objs, caches, modules = watched()
        keep = _tensors(objs) + _tensors([c._vals for c in caches])
        return keep, (tuple(t.data_ptr() for t in keep), _weights_key(modules))

    def stale(self):
        return any(self._fingerprint(w)[1] != fp for (_, w), fp in zip(self._parts, self.fps))

    def replay(self):
        """Replay part after part; False (and nothing more is launched) as soon as a part's buffers or weights are not those of its
        capture.  The parts before it have run then: they write staging and their own buffers only, which a new capture redoes."""
        for (_, watched), graph, fp in zip(self._parts, self.graphs, self.fps):
            if self._fingerprint(watched)[1] != fp:
                return False
            graph.replay()
        return True

    def capture(self, warmup=1):
        dev = self.runner.pool.device
        self._parts = self.parts()
        with torch.cuda.device(dev), torch.no_grad():
            # eager warm-up on a side stream: everything that cannot happen inside a capture happens here (workspaces, weight packs and
            # the host read of their fp16 range check, kernel attributes, the split-K workspace)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):
                    for launch, _ in self._parts:
                        launch()
            torch.cuda.current_stream(dev).wait_stream(side)
            for launch, _ in self._parts:
                graph = torch.cuda.CUDAGraph()
                try:
                    # thread-local capture mode, as GraphedRefine: another thread that polls events must not invalidate this capture
                    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                        self.outs.append(launch())
                except Exception as e:
                    raise MagnetError(f"SequenceRunner(graph=True): capturing the {self.key} step failed: {type(e).__name__}: {e}") from e
                self.graphs.append(graph)
            for _, watched in self._parts:
                keep, fp = self._fingerprint(watched)
                self.keep.append(keep)
                self.fps.append(fp)


class _EncodeGraph(_Captured):
    """add() for n new frames, in two parts.  The D-Net part: the HIP decoder over static copies of the encoder's feature maps (or
    pack_split over a static copy of a torch D-Net's x_d3) into the staging planes.  The F-Net part: the matrix-core F-Net over
    the static images (or pack_features over a static copy of a torch F-Net's output), then one scatter_frames launch through the
    static slot table for everything staged.  The D-Net part goes first: its input (the caller's encoder) is the eager work of a
    step, and while the device runs the decoder the host checks the F-Net part's fingerprint, the larger one by far."""

    def __init__(self, runner, key, src):
        super().__init__(runner, key)
        dev = runner.pool.device
        self.n = src["n"]
        self.static = {k: ([_Static(t, dev, torch.float32) for t in v] if isinstance(v, list) else _Static(v, dev, torch.float32))
                       for k, v in src.items() if k != "n"}
        self.sig = self.signature(src)
        self.table = _TableRing(self.n, dev)
        self._gmm = None

    @staticmethod
    def signature(src):
        return tuple((k, [tuple(t.shape) for t in v] if isinstance(v, list) else tuple(getattr(v, "shape", ()))) for k, v in sorted(src.items()))

    def load(self, src, slots):
        for k, st in self.static.items():
            if isinstance(st, list):
                for s_, t in zip(st, src[k]):
                    s_.load(t)
            else:
                st.load(src[k])
        self.table.push(slots)

    def parts(self):
        return [(self._launch_dnet, self._watched_dnet), (self._launch_fnet, self._watched_fnet)]

    def _launch_dnet(self):
        r = self.runner
        m, n, st = r.model, self.n, self.static
        hi, lo = r._stage_planes(n)
        if "enc" in st:
            feats = [None] * (max(r._dnet_reads) + 1)
            for i, s_ in zip(r._dnet_reads, st["enc"]):
                feats[i] = s_.t
            gmm, _ = m._dnet.run(feats, n_ref=n, x_d3_out=(hi, lo, 256, 0))
        else:
            gmm = st["gmm"].t
            lib.pack_split(st["xd3"].t, hi, lo, 256, 0)      # interior rows; the border rows stay zero
        self._gmm = gmm.detach().float().contiguous()
        return self._gmm

    def _launch_fnet(self):
        r = self.runner
        m, pool, n, st = r.model, r.pool, self.n, self.static
        rows = (pool.h + 2) * (pool.w + 2)
        hi, lo = r._stage_planes(n)
        if "img" in st:
            feat = m._fnet_runner().run(st["img"].t, n_ref=0, feat_dtype=m.feat_dtype)[1]
        else:
            feat = lib.pack_features(st["f"].t, pool.fe, pad=1)
        lib.scatter_frames(self.table.dev, pool_feat=pool.feat, pool_gmm=pool.gmm, pool_xd3=(pool.xd3_hi, pool.xd3_lo),
                           feat=feat, gmm=self._gmm, xd3=(hi.view(n, rows, 256), lo.view(n, rows, 256)))
        return feat

    def _watched_dnet(self):
        r = self.runner
        if "enc" not in self.static:
            return [r._stage], [], []
        d = r.model._dnet
        return [r._stage, d._bufs, d._head_work], [d._cache, d._head._cache], [d.decoder, d._eye]

    def _watched_fnet(self):
        r = self.runner
        pool = r.pool
        objs = [pool.feat, pool.gmm, pool.xd3_hi, pool.xd3_lo, r._stage]
        if "img" not in self.static:
            return objs, [], []
        f = r.model._fnet_runner()
        return objs + [f._bufs], [f._cache], [f.psm]


class _RefineGraph(_Captured):
    """refine() for B windows of V views: gather_views through the static slot table, then match_and_refine on the gathered buffers
    with poses, is_valid and the intrinsics in static device tensors."""

    def __init__(self, runner, key, B, V, mode, poses, is_valid, cam):
        super().__init__(runner, key)
        dev = runner.pool.device
        self.B, self.V, self.mode = B, V, mode
        self.poses = _Static(poses, dev, torch.float32)
        self.is_valid = _Static(is_valid, dev, torch.int32)
        self.cam = {k: _Static(v, dev) for k, v in cam.items()}      # each entry in its own dtype (ray_params are float64)
        self.sig = self.signature(poses, is_valid, cam)
        self.table = _TableRing((1 + V) * B, dev)

    @staticmethod
    def signature(poses, is_valid, cam):
        return (tuple(poses.shape), tuple(is_valid.shape), tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(cam.items())))

    def load(self, table, poses, is_valid, cam):
        self.poses.load(poses)
        self.is_valid.load(is_valid)
        for k, st in self.cam.items():
            st.load(cam[k])
        self.table.push(table)

    def parts(self):
        return [(self._launch, self._watched)]

    def _launch(self):
        r = self.runner
        cam = {k: st.t for k, st in self.cam.items()}
        return r._gather_and_refine(self.table.dev, self.B, self.V, self.poses.t, self.is_valid.t, cam, self.mode)

    def _watched(self):
        r = self.runner
        m, pool = r.model, r.pool
        return ([pool.feat, pool.gmm, pool.xd3_hi, pool.xd3_lo, r._dst.get((self.B, self.V)), m._work],
                [] if m._stacks is None else [st._cache for st in m._stacks], [m.g_net, m.mask_head])


class FramePool:
    """`capacity` slots of one frame's backbone outputs each:
        feat    (capacity, h+2, w+2, F) channel-last F-Net features, zero border, fp32 or bf16
        gmm     (capacity, 2, h, w) fp32 [mu, sigma]
        xd3_hi, xd3_lo (capacity, (h+2)(w+2), 256) split-bf16 planes of x_d3, zero border rows
    and, on the host, the map frame id -> slot in least-recently-used order."""

    def __init__(self, capacity, h, w, F, feat_dtype="fp32", device="cuda"):
        capacity, h, w, F = int(capacity), int(h), int(w), int(F)
        if capacity < 1 or h < 1 or w < 1 or F < 8 or F % 8:
            raise MagnetError(f"FramePool: capacity {capacity}, h {h}, w {w} must be positive and F {F} a multiple of 8")
        self.capacity, self.h, self.w, self.F = capacity, h, w, F
        self.fe = lib.feat_enum(feat_dtype)
        self.device = torch.device(device)
        rows = (h + 2) * (w + 2)
        # zeros: the borders are read by the matcher and the 3x3 convolutions, and no producer writes anything else there
        self.feat = torch.zeros((capacity, h + 2, w + 2, F), dtype=lib.feat_torch_dtype(self.fe), device=self.device)
        self.gmm = torch.zeros((capacity, 2, h, w), dtype=torch.float32, device=self.device)
        self.xd3_hi = torch.zeros((capacity, rows, 256), dtype=torch.bfloat16, device=self.device)
        self.xd3_lo = torch.zeros((capacity, rows, 256), dtype=torch.bfloat16, device=self.device)
        self._slot = OrderedDict()                       # frame id -> slot, least recently used first
        self._free = list(range(capacity))               # never-used slots, handed out in order

    def __len__(self):
        return len(self._slot)

    def __contains__(self, frame_id):
        return frame_id in self._slot

    def ids(self):
        """The frame ids held, least recently used first."""
        return list(self._slot)

    def missing(self, frame_ids):
        """Positions in `frame_ids` of the first occurrence of every id that is not in the pool (None is no frame)."""
        return _first_missing(frame_ids, self._slot)

    def assign(self, frame_ids):
        """Give a slot to every id of `frame_ids` that has none and mark all of them used now.  Free slots go first, in order; then the
        least recently used frame that this call does not name is evicted.  Returns [(position of the id's first occurrence, slot)]
        of the newly assigned ids, in call order: their slots hold another frame's (or no) data until the caller fills them."""
        named = {}                                       # id -> position of its first occurrence, in call order
        for i, fid in enumerate(frame_ids):
            if fid is not None and fid not in named:
                named[fid] = i
        if len(named) > self.capacity:
            raise MagnetError(f"FramePool: the call names {len(named)} distinct frames, the pool holds {self.capacity}")
        new = []
        for fid in named:
            if fid in self._slot:
                self._slot.move_to_end(fid)
                continue
            if self._free:
                slot = self._free.pop(0)
            else:
                victim = next(k for k in self._slot if k not in named)
                slot = self._slot.pop(victim)
            self._slot[fid] = slot
            new.append((named[fid], slot))
        return new

    def release(self, frame_ids):
        """Forget these ids; their slots are free again (what a caller does when it could not fill the slots assign() gave it)."""
        for fid in frame_ids:
            if fid in self._slot:
                self._free.append(self._slot.pop(fid))
        self._free.sort()

    def slots(self, frame_ids):
        """The slot of every id (None -> -1, "no frame"), marking them used now; an id that was never added (or was evicted) raises."""
        out = []
        for fid in frame_ids:
            if fid is None:
                out.append(-1)
                continue
            if fid not in self._slot:
                raise MagnetError(f"FramePool: frame {fid!r} is not in the pool (never added, or evicted: capacity {self.capacity})")
            self._slot.move_to_end(fid)
            out.append(self._slot[fid])
        return out


def slot_table(pool, ref_ids, nghbr_ids):
    """The host form of magnet_gather_views' table for B = len(ref_ids) windows: [b] the slot of window b's reference frame,
    [B + v B + b] the slot of its view v — `nghbr_ids` is in the order of nghbr_imgs, v B + b."""
    B = len(ref_ids)
    if B == 0 or len(nghbr_ids) % B:
        raise MagnetError(f"{len(nghbr_ids)} neighbour ids for {B} reference ids: expected V * B, view-major")
    if any(fid is None for fid in ref_ids):
        raise MagnetError("a reference frame id is None: every window needs its reference frame")
    return pool.slots(list(ref_ids) + list(nghbr_ids))


class SequenceRunner:
    """Inference over a `magnet_amd.magnet.MAGNET` (eval mode, conv_backend='mfma') with the backbones run once per frame.

    add(frame_ids, imgs)    encode the frames the pool does not hold; returns how many were encoded
    refine(...)             one step from frames already in the pool
    forward(...)            add what is missing, then refine: what MAGNET.forward returns for the same windows

    graph=True (opt-in; the default runs every launch eagerly, as before) replays the steps as HIP graphs, for streaming at one new
    frame per step, where the host is what a step waits for.  Results are bit-identical to the eager runner's.
      add()     which frames are missing stays host logic.  A caller's torch modules run eagerly: the D-Net's encoder (HIP D-Net), or
                the whole backbone (torch F-Net / D-Net); their outputs are copied into static tensors.  One graph per (number of new
                frames, image shape), in two parts that replay back to back, then holds the HIP D-Net decoder and the matrix-core
                F-Net (or pack_split / pack_features over the static copies), all writing to staging, and one lib.scatter_frames
                launch through a static slot table.
      refine()  one graph per (B, V, mode) holds lib.gather_views through a static slot table and match_and_refine; poses, is_valid
                (int32) and every cam_intrins entry live in static device tensors.  It returns copies of the graph's output tensors;
                static_outputs=True returns the graph's own tensors, which the next replay of that graph overwrites.
    Before a key's first replay its launches run once eagerly on a side stream (allocations, weight packs and their host-side
    checks), then they are captured; a capture that fails raises MagnetError, there is no fall-back to eager launches.
    A graph bakes in the addresses of the runners' buffers (FNetMFMA, DNetMFMA, MAGNET's workspaces, this runner's staging and gather
    buffers, the pool, the packed weights).  It holds a reference to each of them and a fingerprint (their addresses and the weight
    caches' (data_ptr, _version) keys) that is recomputed on the host before every replay: using the model eagerly with another
    shape, an optimiser step or load_state_dict between two steps costs one new capture, never a wrong answer.  The timing sinks
    (FNetMFMA.event_sink and the like) must be off.  Not captured: the caller's encoder; uint8 ingest.
    image_prep (opt-in; magnet_amd.ingest.ImagePrep or ImagePrepSet): add() and forward() then also take the decoded camera frames,
    uint8 (N, Hin, Win, 3) on the GPU or the host, in place of normalised images.  The frames the pool lacks are selected first and
    only those are prepared, by one eager launch into a buffer of this runner (`prepared` counts them); from there on the step is
    the one above, graph=True included.  uint8 frames without an image_prep raise.
    `graph_stats`: None without graph, else {"captures": {key: count}, "replays": {key: count}} with keys
    ("add", n, image shape) and ("refine", B, V, mode); a step that captures is not counted as a replay."""

    def __init__(self, model, capacity, graph=False, image_prep=None):
        if getattr(model, "conv_backend", None) != "mfma":
            raise MagnetError("SequenceRunner gathers into the matrix-core path's buffers: it needs a MAGNET with conv_backend='mfma'")
        if model.downsample_ratio != 4:
            raise MagnetError(f"SequenceRunner needs downsample_ratio 4 (the matrix-core refinement path), got {model.downsample_ratio}")
        if int(capacity) < 1:
            raise MagnetError(f"SequenceRunner: capacity {capacity} must be at least 1")
        if not isinstance(graph, bool):
            raise MagnetError(f"SequenceRunner: graph must be True or False, got {graph!r}")
        self.model = model
        self.capacity = int(capacity)
        self.pool = None                                 # allocated by the first add(): the backbones decide h, w and F
        self.encoded = 0                                 # images run through the backbones so far
        self._dst = {}                                   # (B, V) -> the gather's destination tensors, reused from call to call
        self._stage = None                               # zero-bordered x_d3 staging planes for the most frames staged so far
        if image_prep is not None and not (callable(getattr(image_prep, "prep", None)) and callable(getattr(image_prep, "check", None))
                                           and hasattr(image_prep, "out_hw")):
            raise MagnetError(f"SequenceRunner: image_prep must be a magnet_amd.ingest.ImagePrep or ImagePrepSet, got {type(image_prep).__name__}")
        self.image_prep = image_prep
        self.prepared = 0                                # uint8 frames run through image_prep so far
        self._prep_buf = None                            # (frames, 3, H, W) fp32: where image_prep writes the new frames of a call
        self.graph = graph
        self.graph_stats = {"captures": {}, "replays": {}} if graph else None
        self._graphs = {}                                # key -> _Captured
        from .dnet import _SKIP_IN, _UP
        self._dnet_reads = (_SKIP_IN,) + tuple(idx for _, idx, _, _ in _UP)   # the encoder outputs the HIP decoder reads

    def _check_inference(self):
        m = self.model
        if torch.is_grad_enabled() and any(p.requires_grad for p in list(m.g_net.parameters()) + list(m.mask_head.parameters())):
            raise MagnetError("SequenceRunner is an inference path: call it under torch.no_grad() (or freeze g_net and mask_head); "
                              "training goes through MAGNET.forward")

    @staticmethod
    def _take_runs(parts, idx):
        """Images `idx` (ascending positions in the concatenation of the tensors `parts`) as slices of `parts`, one per run."""
        out, first = [], 0
        for t in parts:
            n = t.shape[0]
            for _, lo, k in _runs([i - first for i in idx if first <= i < first + n]):
                out.append(t[lo:lo + k])
            first += n
        return out

    @staticmethod
    def _take(parts, idx):
        """Images `idx` as one tensor, by slices only."""
        out = SequenceRunner._take_runs(parts, idx)
        return out[0] if len(out) == 1 else torch.cat(out, dim=0)

    @staticmethod
    def _store(dst, src, slots):
        """src[j] -> dst[slots[j]], one copy per run of consecutive slots."""
        for j, s, k in _runs(slots):
            dst[s:s + k].copy_(src[j:j + k])

    def add(self, frame_ids, imgs):
        """imgs: (N, 3, H, W) on the GPU, or a list of such tensors standing for their concatenation; frame_ids: N ids.  Runs the
        backbones on the images whose id the pool does not hold (the first one of each id) and returns their number."""
        self._check_inference()
        with torch.no_grad():
            return self._add(frame_ids, imgs)

    def _add(self, frame_ids, imgs):
        m = self.model
        parts = list(imgs) if isinstance(imgs, (list, tuple)) else [imgs]
        frame_ids = list(frame_ids)
        if sum(t.shape[0] for t in parts) != len(frame_ids):
            raise MagnetError(f"add: {len(frame_ids)} frame ids for {sum(t.shape[0] for t in parts)} images")
        named = {fid for fid in frame_ids if fid is not None}
        if len(named) > self.capacity:
            raise MagnetError(f"add: the call names {len(named)} distinct frames, the pool holds {self.capacity}")
        raw = any(t.dtype == torch.uint8 for t in parts)
        if raw:
            if self.image_prep is None:
                raise MagnetError("add: uint8 frames need SequenceRunner(..., image_prep=magnet_amd.ingest.ImagePrep(...)); without one the "
                                  "images must be normalised fp32 (N, 3, H, W)")
            if len({(t.dtype, t.device, tuple(t.shape[1:])) for t in parts}) != 1:
                raise MagnetError("add: the uint8 frames of one call must share raw size and device")
            for t in parts:
                self.image_prep.check(t)
        elif any(not t.is_cuda for t in parts):
            raise MagnetError("add: images must be on the GPU (no CPU fallback)")
        idx = self.pool.missing(frame_ids) if self.pool is not None else _first_missing(frame_ids, ())
        if not idx:
            if self.pool is not None:
                self.pool.assign(frame_ids)              # marks them used
            return 0
        if raw:
            sel = self._prepare(self._take_runs(parts, idx))
        else:
            sel = self._take(parts, idx)
        n, dev = sel.shape[0], sel.device
        if self.graph:
            return self._add_graphed(frame_ids, sel)
        # ---- F-Net: the matcher's padded channel-last layout ----
        runner = m._fnet_runner()
        if runner is not None:
            feat = runner.run(sel, n_ref=0, feat_dtype=m.feat_dtype)[1]          # in the runner's own reused buffer
        else:
            feat = lib.pack_features(m.f_net(sel).detach().float().contiguous(), lib.feat_enum(m.feat_dtype), pad=1)
        _, hp, wp, F = feat.shape
        if self.pool is None:
            self.pool = FramePool(self.capacity, hp - 2, wp - 2, F, m.feat_dtype, dev)
        pool = self.pool
        if (hp - 2, wp - 2, F) != (pool.h, pool.w, pool.F) or feat.dtype != pool.feat.dtype or dev != pool.device:
            raise MagnetError(f"add: features {(hp - 2, wp - 2, F)} {feat.dtype} on {dev} do not match the pool's "
                              f"{(pool.h, pool.w, pool.F)} {pool.feat.dtype} on {pool.device}: one pool serves one shape")
        new = pool.assign(frame_ids)
        try:
            self._fill([s for _, s in new], sel, feat)
        except BaseException:
            pool.release([frame_ids[i] for i, _ in new])   # a slot that was not filled must not stay reachable under its new id
            raise
        self.encoded += n
        return n

    def _prepare(self, runs):
        """The uint8 frames the pool lacks (`runs`: slices of the caller's tensors) -> their normalised (n, 3, H, W) images in this
        runner's buffer: one launch.  Several runs of host frames are uploaded run by run into one device tensor (a pinned run without
        blocking): concatenating them on the host first would make a pageable copy."""
        n = sum(t.shape[0] for t in runs)
        host = not runs[0].is_cuda
        dev = runs[0].device if not host else (self.pool.device if self.pool is not None else torch.device(self.image_prep.device))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if len(runs) == 1:
            frames_u8 = runs[0]
        elif host:
            frames_u8 = torch.empty((n,) + tuple(runs[0].shape[1:]), dtype=torch.uint8, device=dev)
            first = 0
            for t in runs:
                frames_u8[first:first + t.shape[0]].copy_(t, non_blocking=t.is_pinned())
                first += t.shape[0]
        else:
            frames_u8 = torch.cat(runs, dim=0)
        buf = self._prep_buf
        if buf is None or buf.shape[0] < n or buf.device != dev or tuple(buf.shape[2:]) != tuple(self.image_prep.out_hw):
            self._prep_buf = None                        # let go of the smaller one first
            buf = self._prep_buf = torch.empty((n, 3) + tuple(self.image_prep.out_hw), dtype=torch.float32, device=dev)
        out = self.image_prep.prep(frames_u8, out=buf[:n])
        self.prepared += n
        return out

    def _stage_planes(self, n):
        """The zero-bordered (n rows, 256) x_d3 staging planes for n frames."""
        rows, dev = n * (self.pool.h + 2) * (self.pool.w + 2), self.pool.device
        if self._stage is None or self._stage[0].shape[0] < rows:
            self._stage = None                           # let go of the smaller pair first
            self._stage = (torch.zeros((rows, 256), dtype=torch.bfloat16, device=dev),
                           torch.zeros((rows, 256), dtype=torch.bfloat16, device=dev))
        return self._stage[0][:rows], self._stage[1][:rows]

    def _add_graphed(self, frame_ids, sel):
        """add() in graph mode for the new images `sel`: the caller's torch modules eagerly, the rest as replayed graphs."""
        m = self.model
        n, dev = sel.shape[0], sel.device
        src = {"n": n}
        f_run = m._fnet_runner()
        if f_run is not None:
            src["img"] = sel
            H, W = sel.shape[2:]
            h, w = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
            if self.pool is None:
                f_run.packed(dev)                        # the weight pack knows the feature width
            F = f_run.feature_dim if self.pool is None else self.pool.F      # (the scatter checks the staged features against the pool)
        else:
            src["f"] = m.f_net(sel).detach().float().contiguous()
            _, F, h, w = src["f"].shape
        if self.pool is None:
            self.pool = FramePool(self.capacity, h, w, F, m.feat_dtype, dev)
        pool = self.pool
        if (h, w, F) != (pool.h, pool.w, pool.F) or dev != pool.device:
            raise MagnetError(f"add: features {(h, w, F)} on {dev} do not match the pool's {(pool.h, pool.w, pool.F)} on {pool.device}: "
                              "one pool serves one shape")
        new = pool.assign(frame_ids)
        try:
            if m.dnet_backend == "hip" and not m.d_net.training:
                feats = m.d_net.d_net.encoder(sel)
                if tuple(feats[5].shape[2:]) != (pool.h, pool.w):
                    raise MagnetError(f"add: the D-Net works at {tuple(feats[5].shape[2:])}, the F-Net at {(pool.h, pool.w)}")
                src["enc"] = [feats[i] for i in self._dnet_reads]
            else:
                gmm, x_d3 = m.d_net(sel)
                if x_d3.shape[1] != 256 or tuple(x_d3.shape[2:]) != (pool.h, pool.w) or tuple(gmm.shape[1:]) != (2, pool.h, pool.w):
                    raise MagnetError(f"add: the D-Net gave (mu, sigma) {tuple(gmm.shape)} and x_d3 {tuple(x_d3.shape)}; the pool takes "
                                      f"(N, 2, {pool.h}, {pool.w}) and (N, 256, {pool.h}, {pool.w})")
                src["gmm"], src["xd3"] = gmm, x_d3
            key = ("add", n, tuple(sel.shape[1:]))
            sig = _EncodeGraph.signature(src)
            self._step(key, sig, lambda: _EncodeGraph(self, key, src), lambda g: g.load(src, [s for _, s in new]))
        except BaseException:
            pool.release([frame_ids[i] for i, _ in new])   # a slot that was not filled must not stay reachable under its new id
            raise
        self.encoded += n
        return n

    def _step(self, key, sig, make, load):
        """Replay the graphs of `key` on inputs set by load(graphs); capture them first where there are none, their static tensors have
        another form (`sig`), or a buffer or weight they read has changed since the capture."""
        stats = self.graph_stats
        g = self._graphs.get(key)
        if g is not None and g.sig != sig:
            del self._graphs[key]
            g = None
        if g is not None:
            load(g)
            if g.replay():
                stats["replays"][key] = stats["replays"].get(key, 0) + 1
                return g
            del self._graphs[key]                        # stale
        g = make()
        load(g)
        g.capture()
        self._graphs[key] = g
        stats["captures"][key] = stats["captures"].get(key, 0) + 1
        stats["replays"].setdefault(key, 0)
        # the runners keep one shape's buffers at a time: graphs whose buffers this capture has displaced hold memory for nothing
        for k in [k for k, o in self._graphs.items() if o is not g and o.stale()]:
            del self._graphs[k]
        if not g.replay():
            raise MagnetError(f"SequenceRunner(graph=True): the {key} step changed its own buffers between its capture and its first replay")
        return g

    def _fill(self, slots, sel, feat):
        """The backbone outputs of the images `sel` into the pool's `slots` (`feat`: their F-Net features, already computed)."""
        m, pool = self.model, self.pool
        n, dev = sel.shape[0], sel.device
        self._store(pool.feat, feat, slots)
        # ---- D-Net: (mu, sigma) and the split-bf16 x_d3 planes ----
        rows = (pool.h + 2) * (pool.w + 2)
        one_run = slots == list(range(slots[0], slots[0] + n))
        if one_run:                                      # consecutive slots: the producers write straight into the pool
            hi, lo = pool.xd3_hi[slots[0]:slots[0] + n].view(n * rows, 256), pool.xd3_lo[slots[0]:slots[0] + n].view(n * rows, 256)
        else:
            hi, lo = self._stage_planes(n)
        if m.dnet_backend == "hip" and not m.d_net.training:
            feats = m.d_net.d_net.encoder(sel)
            if tuple(feats[5].shape[2:]) != (pool.h, pool.w):
                raise MagnetError(f"add: the D-Net works at {tuple(feats[5].shape[2:])}, the F-Net at {(pool.h, pool.w)}")
            gmm, _ = m._dnet.run(feats, n_ref=n, x_d3_out=(hi, lo, 256, 0))
        else:
            gmm, x_d3 = m.d_net(sel)
            if x_d3.shape[1] != 256 or tuple(x_d3.shape[2:]) != (pool.h, pool.w) or tuple(gmm.shape[1:]) != (2, pool.h, pool.w):
                raise MagnetError(f"add: the D-Net gave (mu, sigma) {tuple(gmm.shape)} and x_d3 {tuple(x_d3.shape)}; the pool takes "
                                  f"(N, 2, {pool.h}, {pool.w}) and (N, 256, {pool.h}, {pool.w})")
            lib.pack_split(x_d3.detach().float().contiguous(), hi, lo, 256, 0)   # interior rows; the border rows stay zero
        if not one_run:
            self._store(pool.xd3_hi, hi.view(n, rows, 256), slots)
            self._store(pool.xd3_lo, lo.view(n, rows, 256), slots)
        self._store(pool.gmm, gmm.detach().float(), slots)

    def slot_table(self, ref_ids, nghbr_ids):
        if self.pool is None:
            raise MagnetError(f"refine: frame {list(ref_ids)[0] if len(ref_ids) else None!r} is not in the pool (nothing was added yet)")
        return slot_table(self.pool, list(ref_ids), list(nghbr_ids))

    def refine(self, ref_ids, nghbr_ids, nghbr_poses, is_valid, cam_intrins, mode="test", static_outputs=False):
        """One step over frames already in the pool: `ref_ids` (B), `nghbr_ids` (V B, in the order of nghbr_imgs: v B + b).  Returns
        what MAGNET.forward returns.  Graph mode returns copies of the graph's output tensors; with static_outputs=True it returns the
        graph's own tensors, valid until the next replay of the same (B, V, mode) graph (no copy).  Without graph the flag changes
        nothing: every call returns fresh tensors."""
        self._check_inference()
        table = self.slot_table(ref_ids, nghbr_ids)
        with torch.no_grad():
            if self.graph:
                return self._refine_graphed(table, len(ref_ids), nghbr_poses, is_valid, cam_intrins, mode, static_outputs)
            return self._refine(table, len(ref_ids), nghbr_poses, is_valid, cam_intrins, mode)

    def _refine_graphed(self, table, B, poses, is_valid, cam, mode, static_outputs):
        if missing := [n_ for n_, v in (("nghbr_poses", poses), ("is_valid", is_valid), ("cam_intrins", cam)) if v is None]:
            raise MagnetError(f"refine: {', '.join(missing)} missing")
        V = len(table) // B - 1
        key = ("refine", B, V, mode)
        sig = _RefineGraph.signature(poses, is_valid, cam)
        g = self._step(key, sig, lambda: _RefineGraph(self, key, B, V, mode, poses, is_valid, cam),
                       lambda g: g.load(table, poses, is_valid, cam))
        return list(g.out) if static_outputs else [p.clone() for p in g.out]

    def _refine(self, table, B, nghbr_poses, is_valid, cam_intrins, mode):
        V = len(table) // B - 1
        slots = torch.tensor(table, dtype=torch.int32).pin_memory().to(self.pool.device, non_blocking=True)
        return self._gather_and_refine(slots, B, V, nghbr_poses, is_valid, cam_intrins, mode)

    def _gather_and_refine(self, slots, B, V, nghbr_poses, is_valid, cam_intrins, mode):
        m, pool = self.model, self.pool
        dev, h, w = pool.device, pool.h, pool.w
        dst = self._dst.get((B, V))
        if dst is None:
            self._dst.clear()                            # one step shape at a time: the buffers are large
            dst = self._dst[(B, V)] = (torch.empty((B, h, w, pool.F), dtype=pool.feat.dtype, device=dev),
                                       torch.empty((V * B, h + 2, w + 2, pool.F), dtype=pool.feat.dtype, device=dev),
                                       torch.empty((B, 2, h, w), dtype=torch.float32, device=dev),
                                       torch.empty((V * B, 2, h, w), dtype=torch.float32, device=dev))
        ref_cl, src_pad, ref_gmm, src_gmm = dst
        lib.gather_views(slots, B, V, pool_feat=pool.feat, pool_gmm=pool.gmm, pool_xd3=(pool.xd3_hi, pool.xd3_lo),
                         ref_cl=ref_cl, src_pad=src_pad, ref_gmm=ref_gmm, src_gmm=src_gmm, gin=m.gnet_input_buffer(B, h, w, dev))
        return m.match_and_refine(ref_gmm, None, None, None, src_gmm, nghbr_poses, is_valid, cam_intrins, mode,
                                  packed_feats=(ref_cl, src_pad), x_d3_in_place=True)

    def forward(self, ref_ids, ref_img, nghbr_ids, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, mode="test", static_outputs=False):
        """MAGNET.forward with frame ids: ref_ids (B) name the images of ref_img, nghbr_ids (V B) those of nghbr_imgs."""
        self.add(list(ref_ids) + list(nghbr_ids), [ref_img, nghbr_imgs])
        return self.refine(ref_ids, nghbr_ids, nghbr_poses, is_valid, cam_intrins, mode, static_outputs)
