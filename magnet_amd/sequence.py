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
    forward(...)            add what is missing, then refine: what MAGNET.forward returns for the same windows"""

    def __init__(self, model, capacity):
        if getattr(model, "conv_backend", None) != "mfma":
            raise MagnetError("SequenceRunner gathers into the matrix-core path's buffers: it needs a MAGNET with conv_backend='mfma'")
        if model.downsample_ratio != 4:
            raise MagnetError(f"SequenceRunner needs downsample_ratio 4 (the matrix-core refinement path), got {model.downsample_ratio}")
        if int(capacity) < 1:
            raise MagnetError(f"SequenceRunner: capacity {capacity} must be at least 1")
        self.model = model
        self.capacity = int(capacity)
        self.pool = None                                 # allocated by the first add(): the backbones decide h, w and F
        self.encoded = 0                                 # images run through the backbones so far
        self._dst = {}                                   # (B, V) -> the gather's destination tensors, reused from call to call
        self._stage = None                               # zero-bordered x_d3 staging planes for the most frames staged so far

    def _check_inference(self):
        m = self.model
        if torch.is_grad_enabled() and any(p.requires_grad for p in list(m.g_net.parameters()) + list(m.mask_head.parameters())):
            raise MagnetError("SequenceRunner is an inference path: call it under torch.no_grad() (or freeze g_net and mask_head); "
                              "training goes through MAGNET.forward")

    @staticmethod
    def _take(parts, idx):
        """Images `idx` (ascending positions in the concatenation of the tensors `parts`) as one tensor, by slices only."""
        out, first = [], 0
        for t in parts:
            n = t.shape[0]
            for _, lo, k in _runs([i - first for i in idx if first <= i < first + n]):
                out.append(t[lo:lo + k])
            first += n
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
        if any(not t.is_cuda for t in parts):
            raise MagnetError("add: images must be on the GPU (no CPU fallback)")
        idx = self.pool.missing(frame_ids) if self.pool is not None else _first_missing(frame_ids, ())
        if not idx:
            if self.pool is not None:
                self.pool.assign(frame_ids)              # marks them used
            return 0
        sel = self._take(parts, idx)
        n, dev = sel.shape[0], sel.device
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
            if self._stage is None or self._stage[0].shape[0] < n * rows:
                self._stage = None                       # let go of the smaller pair first
                self._stage = (torch.zeros((n * rows, 256), dtype=torch.bfloat16, device=dev),
                               torch.zeros((n * rows, 256), dtype=torch.bfloat16, device=dev))
            hi, lo = self._stage[0][:n * rows], self._stage[1][:n * rows]
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

    def refine(self, ref_ids, nghbr_ids, nghbr_poses, is_valid, cam_intrins, mode="test"):
        """One step over frames already in the pool: `ref_ids` (B), `nghbr_ids` (V B, in the order of nghbr_imgs: v B + b).  Returns
        what MAGNET.forward returns."""
        self._check_inference()
        table = self.slot_table(ref_ids, nghbr_ids)
        with torch.no_grad():
            return self._refine(table, len(ref_ids), nghbr_poses, is_valid, cam_intrins, mode)

    def _refine(self, table, B, nghbr_poses, is_valid, cam_intrins, mode):
        m, pool = self.model, self.pool
        V = len(table) // B - 1
        dev, h, w = pool.device, pool.h, pool.w
        slots = torch.tensor(table, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
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

    def forward(self, ref_ids, ref_img, nghbr_ids, nghbr_imgs, nghbr_poses, is_valid, cam_intrins, mode="test"):
        """MAGNET.forward with frame ids: ref_ids (B) name the images of ref_img, nghbr_ids (V B) those of nghbr_imgs."""
        self.add(list(ref_ids) + list(nghbr_ids), [ref_img, nghbr_imgs])
        return self.refine(ref_ids, nghbr_ids, nghbr_poses, is_valid, cam_intrins, mode)
