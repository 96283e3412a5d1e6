"""Runs the reference's small conv stacks (GNET.gnet, mask_head — models/MAGNET.py:51-56,111-116:
Conv3x3(pad 1)-ReLU-Conv1x1-ReLU-Conv1x1-ReLU-Conv1x1) on the bf16x3 MFMA kernel (csrc/conv_mfma.hip).

Activations are zero-bordered channel-last buffers (B, h+2, w+2, C) kept as two bf16 planes (hi, lo); the
weights of the nn.Conv2d modules are re-packed (and re-split) lazily whenever a parameter changes, so the
module keeps its reference state_dict and stays trainable through the torch path.
"""
from __future__ import annotations

import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lib
from .planes import PackCache, pack_taps, pack_taps_f16, planes, round_up, split_bf16, timed


def _cout_pad(c):
    if c <= 16:
        return 16
    if c == 144:
        return 144
    return round_up(c, 128)


# Latency mode.  Under small_tiles = "auto" a 3x3 launch of a stack whose 128-row tiling has fewer than SMALL_TILE_LIMIT tiles goes to
# the 64-row instance (lib.TILING_BM64: twice the workgroups, bit-identical results).  The natural limit would be 256, the CUs of an MI355X:
# below it the 128-row form leaves CUs without work and the others with one workgroup of a kernel built for two.  Measured
# (profiles/latency/NOTES.md): at one frame of 120 x 160 (152 tiles) the replayed shipped step gains in 12 of 12 interleaved pairs
# (0.2938 vs 0.2986 ms) and the C2 step in 1 (0.1882 vs 0.1874 ms), launched eagerly (host-bound) in 2 and 2; one KITTI frame (211 tiles)
# loses in every pair, and so do two and three frames (304, 456 tiles) — a CU's critical path is 128 rows either way.
# The bar is every pair at every workload measured, so the limit is 0: "auto" keeps the 128-row launches and the 64-row form is opt-in (small_tiles = True).
SMALL_TILE_LIMIT = 0


@functools.lru_cache(maxsize=None)
def tiles_128(n_img, h, wp, by_image=True):
    """128-row tiles of a 3x3 launch over n_img zero-bordered (h + 2, wp) grids: what magnet_conv_row_tiles says for the launches that
    know their image geometry (fused Gaussian update / upsampling), the flat count ceil(rows / 128) for the others."""
    if by_image:
        return lib.conv_row_tiles(n_img, h, wp, 128)[0]
    return (n_img * (h + 2) * wp + 127) // 128


def use_small_tiles(n_img, h, wp, by_image=True):
    """The rule of ConvStackMFMA.small_tiles == "auto": one threshold on the 128-row tile count.  Pure host arithmetic."""
    return tiles_128(n_img, h, wp, by_image) < SMALL_TILE_LIMIT


def _tile_rows(n, small, rows, wp, geom):
    """Tile rows of a launch from the tile count n the library reported for it: 64 under TILING_BM64, else the one of the library's
    own 128- and 256-row forms whose tiling of the launch (magnet_conv_row_tiles where the launch carries its image geometry, else
    rows / tile rows rounded up) has n tiles.  Nothing of launch_conv_mfma's selection is restated here."""
    for bm in ((64,) if small else (128, 256)):
        if n == (lib.conv_row_tiles(*geom, wp, bm)[0] if geom is not None else -(-rows // bm)):
            return bm
    raise lib.MagnetError(f"ConvStackMFMA: {n} row tiles reported for {rows} rows match no tile form")


def _buf(work, key, make):
    """work[key], made on first use."""
    if key not in work:
        work[key] = make()
    return work[key]


class ConvStackMFMA:
    """`seq`: nn.Sequential of Conv2d / ReLU as in the reference.  `in_map`: how the first layer's input channels are
    laid out in the (wider, 32-aligned) input buffer: list of (src_start, length, dst_start)."""

    # When set to a list, every layer launch appends (start_event, end_event, flops, taps) recorded on the launch
    # stream (bench.py's live timing of the convolution kernel).
    event_sink = None

    # Tile form of the stack's 3x3 launches (class default; set on an instance to override): "auto" = 64-row tiles when
    # use_small_tiles() says the 128-row form under-fills the chip, True = always where a 64-row instance exists, False = never.
    # Results do not depend on it, bit for bit.
    small_tiles = "auto"
    # True: every 3x3 launch goes through magnet_conv_mfma_ex and last_tiles / last_invariant_tiles hold [(tile rows, row tiles)] of
    # the last run() / run_invariant(), as the library reported them (tests, tools).  Off by default: a one-frame step launched eagerly
    # is host-bound, and a launch that keeps its tile form is then exactly the magnet_conv_mfma call it was before the 64-row form
    # existed.  A launch on 64-row tiles is recorded either way.
    record_tiles = False
    # True: the fused-tail 3x3 launches take the 256-row 8-wave kernel at any row count (lib.TILING_BM256), which the library itself
    # selects from 65 536 rows on: the tests reach that kernel, and run(src_nchw=...), with small grids.  Not with small_tiles=True.
    tile_256 = False
    last_tiles = ()
    last_invariant_tiles = ()

    def _tiling(self, pk, rows, wp, gauss=None, upsample=None):
        """(tiling, geom) of the launch of this stack's first layer `pk` over `rows` rows of pitch wp.  tiling, the argument of
        lib.conv_mfma: lib.TILING_BM64, 0 (the library chooses; the count is reported) or None (magnet_conv_mfma: nothing reported).
        geom = (n_img, h) where the launch carries its image geometry (gauss / upsample), else None.  The one place that says
        whether there is anything to decide or record: in the common case (no) this is two attribute reads and a comparison."""
        st = self.small_tiles
        if pk["taps"] != 9 or not (self.record_tiles or self.tile_256 or st is True or (st == "auto" and SMALL_TILE_LIMIT > 0)):
            return None, None
        geom = self._geom(gauss, upsample)
        if st is not False and pk["cout_pad"] % 128 == 0 and \
                (st is True or (use_small_tiles(*geom, wp) if geom is not None else use_small_tiles(1, rows // wp - 2, wp, False))):
            return lib.TILING_BM64, geom
        if self.tile_256 and (gauss is not None or upsample is not None):
            return lib.TILING_BM256, geom
        return (0 if self.record_tiles else None), geom

    @staticmethod
    def _geom(gauss, upsample):
        """(n_img, h) of a launch that carries its image geometry (gauss / upsample), else None."""
        return (int(gauss[0].shape[0]), int(gauss[0].shape[2])) if gauss is not None else \
            (int(upsample[0].shape[1]), int(upsample[0].shape[3])) if upsample is not None else None

    @staticmethod
    def _reported(n, tiling, rows, wp, geom):
        """last_tiles of one launch whose tile count n the library reported: [(tile rows, row tiles)]."""
        return [(_tile_rows(n, bool(tiling) and bool(tiling & lib.TILING_BM64), rows, wp, geom), n)]

    def __init__(self, seq: nn.Sequential, in_map=None):
        self.layers = []
        mods = list(seq)
        i = 0
        while i < len(mods):
            conv = mods[i]
            if not isinstance(conv, nn.Conv2d):
                raise lib.MagnetError(f"ConvStackMFMA: unexpected module {type(conv).__name__}")
            k = conv.kernel_size
            if k not in ((1, 1), (3, 3)) or conv.stride != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 or \
                    conv.padding != ((k[0] - 1) // 2, (k[1] - 1) // 2):
                raise lib.MagnetError("ConvStackMFMA supports 1x1 and 3x3 (pad 1) stride-1 convolutions")
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            self.layers.append((conv, relu))
            i += 2 if relu else 1
        self.in_map = in_map
        # The stack's three 1x1 layers fused into the EPILOGUE of its first (3x3) layer: the 128 x 128 tile is already
        # on the CU, weights come straight from L2, LDS need stays at the K ring's 64 KB (2 workgroups per CU).
        # False: one launch per layer.
        self.fuse_epilogue = True
        self._chain = None
        self._cache = PackCache(lambda: [p for conv, _ in self.layers for p in conv.parameters()])

    def can_fuse_gauss(self, device):
        """True when run(..., gauss=...) is available: the reference's G-Net (3x3 + three 1x1, 2 outputs) with the fused epilogue on."""
        self.packed(device)
        return self._chain is not None and self.fuse_epilogue and self._chain["cout_pad"] == 16

    def can_fuse_upsample(self, device):
        """True when run(..., upsample=...) is available: the reference's mask head (3x3 + three 1x1, 9 * 16 outputs) with the fused
        epilogue on."""
        self.packed(device)
        return self._chain is not None and self.fuse_epilogue and self._chain["cout_pad"] == 144

    def cin_pad(self):
        c0 = self.layers[0][0].in_channels
        if self.in_map is None:
            return round_up(c0, 32)
        return round_up(max(d + n for _, n, d in self.in_map), 32)

    def _first_weight(self, device):
        """The first layer's fp32 weight (cout, cin, kh, kw) with its input channels laid out as the input buffer has them (in_map)."""
        W = self.layers[0][0].weight.detach().to(device=device, dtype=torch.float32)
        if self.in_map is None:
            return W
        Wm = torch.zeros((W.shape[0], self.cin_pad()) + tuple(W.shape[2:]), dtype=torch.float32, device=device)
        for src, n, dst in self.in_map:
            Wm[:, dst:dst + n] = W[:, src:src + n]
        return Wm

    def packed(self, device):
        """Per layer the padded split-bf16 weights, the bias and the launch geometry; the repack also rebuilds (or drops) _chain."""
        return self._cache.get(device, lambda: self._pack(device))

    @torch.no_grad()
    def _pack(self, device):
        out = []
        cin_p = self.cin_pad()
        for li, (conv, relu) in enumerate(self.layers):
            W = self._first_weight(device) if li == 0 else conv.weight.detach().to(device=device, dtype=torch.float32)   # (Cout, Cin, kh, kw)
            cout, cin, kh, kw = W.shape
            cp = _cout_pad(cout)
            hi, lo = (F.pad(t, (0, 0, 0, cp - cout)) for t in pack_taps(W, cin_p))   # (tap, cout_pad, cin_pad)
            bias = torch.zeros(cp, dtype=torch.float32, device=device)
            if conv.bias is not None:
                bias[:cout] = conv.bias.detach().to(device=device, dtype=torch.float32)
            out.append(dict(w_hi=hi, w_lo=lo, bias=bias, taps=kh * kw, cin=cin_p, cout=cout, cout_pad=cp, relu=relu))
            cin_p = cp                                                                 # next layer reads all padded channels
            if li + 1 < len(self.layers) and cp % 32 != 0:
                raise lib.MagnetError("hidden layer width must be a multiple of 32")
        # the reference's stacks end in 1x1(128->128)+ReLU, 1x1(128->128)+ReLU, 1x1(128->cout): the fused tail's weights
        self._chain = None
        if len(out) == 4 and all(o["taps"] == 1 for o in out[1:]) and out[1]["relu"] and out[2]["relu"] and \
                not out[3]["relu"] and out[0]["cout_pad"] == 128 and out[1]["cout_pad"] == 128 and \
                out[2]["cout_pad"] == 128 and out[3]["cout_pad"] in (16, 128, 144) and out[0]["relu"]:
            self._chain = dict(
                w_hi=torch.cat([o["w_hi"].reshape(-1) for o in out[1:]]).contiguous(),
                w_lo=torch.cat([o["w_lo"].reshape(-1) for o in out[1:]]).contiguous(),
                bias=torch.cat([o["bias"] for o in out[1:]]).contiguous(), cout_pad=out[3]["cout_pad"])
        return out

    def packed_f16(self, device, n_var=None, inv_off=None):
        """First layer's weights as ONE fp16 plane (taps, cout_pad, cin), rounded once from the fp32 parameter (planes.pack_taps_f16):
        the weight operand of the single-plane fp16 format.  With n_var / inv_off: (variable part, invariant part) over the channels
        packed_first_split() cuts — buffer channels [0, round_up(n_var, 32)) and [inv_off, cin_pad)."""
        @torch.no_grad()
        def build():
            pk = self.packed(device)[0]
            w = F.pad(pack_taps_f16(self._first_weight(device), pk["cin"]), (0, 0, 0, pk["cout_pad"] - pk["cout"]))
            if n_var is None:
                return w
            cv = round_up(n_var, 32)
            wv = w[:, :, :cv].clone(); wv[:, :, n_var:] = 0
            return wv.contiguous(), w[:, :, inv_off:].contiguous()
        return self._cache.get(device, build, "f16", n_var, inv_off)

    def packed_first_split(self, device, n_var, inv_off):
        """First layer split by input channels of the (padded) input buffer: channels [0, n_var) vary per refinement
        iteration (the cost volume), channels [inv_off, cin_pad) are loop-invariant (x_d3), everything between is padding.
        Returns (variable part, invariant part): variable = weights over buffer channels [0, round_up(n_var,32)) (+ bias,
        ReLU); invariant = weights over buffer channels [inv_off, cin_pad) only — its launch reads the buffer at a channel
        offset, so no MFMA work is spent on the cost channels' zero weights (no bias, no ReLU)."""
        @torch.no_grad()
        def build():
            pk = self.packed(device)[0]
            if inv_off % 32 or inv_off < n_var:
                raise lib.MagnetError("packed_first_split: the invariant channels must start at a multiple of 32 behind the variable ones")
            w = (pk["w_hi"].float() + pk["w_lo"].float())                       # exact: hi + lo is how the kernel sees them
            cv = round_up(n_var, 32)
            wv = w[:, :, :cv].clone(); wv[:, :, n_var:] = 0
            wi = w[:, :, inv_off:].clone()
            # re-splitting hi + lo is exact (16 mantissa bits): hi, lo are recovered bit for bit
            vh, vl = split_bf16(wv.contiguous()); ih, il = split_bf16(wi.contiguous())
            var = dict(w_hi=vh, w_lo=vl, bias=pk["bias"], taps=pk["taps"], cin=cv, cout_pad=pk["cout_pad"], relu=pk["relu"])
            inv = dict(w_hi=ih, w_lo=il, bias=torch.zeros_like(pk["bias"]), taps=pk["taps"], cin=pk["cin"] - inv_off,
                       cout_pad=pk["cout_pad"], relu=False)
            return var, inv
        return self._cache.get(device, build, "split", n_var, inv_off)

    def run_invariant(self, in_hi, in_lo, in_ld, rows, wp, work, n_var, inv_off, f16=False):
        """Loop-invariant partial sums of the first layer: fp32 (rows, cout_pad), computed once per forward.  in_hi / in_lo:
        channel 0 of the buffer; the launch starts at channel inv_off.
        f16 = True: in_hi is the fp16 plane of the single-plane fp16 format and in_lo is None (see run())."""
        if f16:
            self._check_f16(in_hi, in_lo)
        _, inv = self.packed_first_split(in_hi.device, n_var, inv_off)
        out = _buf(work, ("partial", rows, inv["cout_pad"]), lambda: torch.empty((rows, inv["cout_pad"]), dtype=torch.float32, device=in_hi.device))
        if f16:
            n = lib.conv_mfma(in_hi[:, inv_off:], None, in_ld, inv["cin"], self.packed_f16(in_hi.device, n_var, inv_off)[1], None, inv["bias"],
                              inv["taps"], wp, False, rows, out_f32=out, f16=True)
            self.last_invariant_tiles = self._reported(n, False, rows, wp, None) if self.record_tiles else ()
            return out
        tiling, geom = self._tiling(inv, rows, wp)
        n = lib.conv_mfma(in_hi[:, inv_off:], in_lo[:, inv_off:], in_ld, inv["cin"], inv["w_hi"], inv["w_lo"], inv["bias"], inv["taps"], wp,
                          False, rows, out_f32=out, tiling=tiling)
        self.last_invariant_tiles = () if n is None else self._reported(n, tiling, rows, wp, geom)
        return out

    def _check_f16(self, in_hi, in_lo):
        if self.small_tiles is True:
            raise lib.MagnetError("ConvStackMFMA: the single-plane fp16 format has no 64-row tile form (small_tiles=True)")
        if in_lo is not None or in_hi.dtype != torch.float16:
            raise lib.MagnetError("ConvStackMFMA: f16=True takes one fp16 plane (in_hi) and in_lo=None")

    def run(self, in_hi, in_lo, in_ld, rows, wp, work, first_addend=None, n_var=None, inv_off=None, upsample=None, gauss=None, f16=False,
            src_nchw=None):
        """in_hi/in_lo: bf16 views whose data_ptr is row 0, channel 0 of this stack's input; `work`: dict for cached
        hidden buffers.  Returns (fp32 tensor (rows, cout_pad_last), cout_pad_last).
        upsample = (depths (n,B,2,h,w), outs (n,B,2,4h,4w)): the mask head's stack only (144 outputs, fused tail) — the learned
        convex upsampling runs in the tail's last layer and only `outs` is written (returns (None, 144)); see can_fuse_upsample().
        gauss = (gmm_in, gmm_out): G-Net's stack only — the Gaussian update runs behind the head (returns (None, 16)); can_fuse_gauss().
        f16 = True: the 3x3 layer on the single-plane fp16 format (lib.conv_mfma(f16=True)): in_hi is an fp16 plane, in_lo None; the
        fused 1x1 tail stays bf16x3.  Fused-epilogue stacks only; with small_tiles=True a MagnetError (no 64-row form).
        src_nchw = (x (B, C, h, w) fp32, c0): the first layer's input channels [c0, c0 + C) are read in place from x
        (lib.conv_mfma(src_nchw=...): the planes' channels from c0 on are not read; in_hi / in_lo may be None when c0 == 0).  Fused-
        epilogue stacks with gauss or upsample, bf16x3, no first_addend; the library refuses what its entry point does not serve."""
        dev = in_hi.device if in_hi is not None else src_nchw[0].device
        if src_nchw is not None:
            self.packed(dev)
            if f16 or first_addend is not None or (gauss is None and upsample is None) or self._chain is None or \
                    not self.fuse_epilogue:
                raise lib.MagnetError("ConvStackMFMA.run (src_nchw): the bf16x3 fused-epilogue launch with gauss or upsample only")
        packs = self.packed(dev)
        if f16:
            self._check_f16(in_hi, in_lo)
            if self._chain is None or not self.fuse_epilogue or self._chain["cout_pad"] not in (16, 144):
                raise lib.MagnetError("ConvStackMFMA.run(f16=True): needs the fused-epilogue stack of G-Net or the mask head")
        if first_addend is not None:
            # first layer over the per-iteration channels only; the invariant part arrives as `first_addend`
            packs = [self.packed_first_split(dev, n_var, inv_off)[0]] + list(packs[1:])
        sink = ConvStackMFMA.event_sink
        # the stack's first layer (its one 3x3 launch) takes its tile form from small_tiles; tiling None is the plain entry point.
        # The fp16 entry point takes no tiling and always reports its tile count: recorded under record_tiles
        tiling, geom = (None, self._geom(gauss, upsample)) if f16 else self._tiling(packs[0], rows, wp, gauss, upsample)
        self.last_tiles = ()

        def out_f32(c):
            return _buf(work, ("out", rows, c), lambda: torch.empty((rows, c), dtype=torch.float32, device=dev))

        def flops(pk):
            return 2.0 * rows * pk["cout_pad"] * pk["cin"] * pk["taps"]

        if self._chain is not None and self.fuse_epilogue:
            pk, ch = packs[0], self._chain
            out = None if (upsample is not None or gauss is not None) else out_f32(ch["cout_pad"])
            w_hi, w_lo = pk["w_hi"], pk["w_lo"]
            if f16:                                       # one fp16 weight plane; the fused 1x1 tail stays bf16x3
                w_hi, w_lo = (self.packed_f16(dev) if first_addend is None else self.packed_f16(dev, n_var, inv_off)[0]), None
            with timed(sink, flops(pk) + 2.0 * rows * 128 * (256 + ch["cout_pad"]), pk["taps"]):
                n = lib.conv_mfma(in_hi, in_lo, in_ld, pk["cin"], w_hi, w_lo, pk["bias"], pk["taps"], wp, pk["relu"], rows, out_f32=out,
                                  tail=(ch["w_hi"], ch["w_lo"], ch["bias"], ch["cout_pad"]), upsample=upsample, gauss=gauss, tiling=tiling,
                                  src_nchw=src_nchw, addend=first_addend, f16=bool(f16))
            # (the src_nchw entry point always reports its tile count; it is recorded where the plain launch's would be)
            recorded = self.record_tiles if f16 else tiling is not None
            self.last_tiles = self._reported(n, tiling, rows, wp, geom) if n is not None and recorded else ()
            return out, ch["cout_pad"]
        cur_hi, cur_lo, cur_ld = in_hi, in_lo, in_ld
        for li, pk in enumerate(packs[:-1]):
            oh, ol = _buf(work, ("hid", li & 1, rows, pk["cout_pad"]), lambda: planes(rows, pk["cout_pad"], dev))
            with timed(sink, flops(pk), pk["taps"]):
                n = lib.conv_mfma(cur_hi, cur_lo, cur_ld, pk["cin"], pk["w_hi"], pk["w_lo"], pk["bias"], pk["taps"], wp,
                                  pk["relu"], rows, out_hi=oh, out_lo=ol, addend=first_addend if li == 0 else None,
                                  tiling=tiling if li == 0 else None)
            if li == 0:
                self.last_tiles = () if n is None else self._reported(n, tiling, rows, wp, geom)
            cur_hi, cur_lo, cur_ld = oh, ol, pk["cout_pad"]
        pk = packs[-1]
        out = out_f32(pk["cout_pad"])
        with timed(sink, flops(pk), pk["taps"]):
            lib.conv_mfma(cur_hi, cur_lo, cur_ld, pk["cin"], pk["w_hi"], pk["w_lo"], pk["bias"], pk["taps"], wp,
                          pk["relu"], rows, out_f32=out)
        return out, pk["cout_pad"]
