"""The D-Net's encoder: EfficientNet-B5 (`tf_efficientnet_b5`) written out here, so that no `torch.hub` download and no extra package
is needed (reference: models/submodules/D_dense_depth.py:7-25, which loads 'rwightman/gen-efficientnet-pytorch').

Two things live here, as in fnet.py:

* `Encoder` / `GenEfficientNetB5`: plain nn.Modules with the GenEfficientNet attribute structure and **state_dict keys**
  (`original_model.conv_stem.weight`, `original_model.blocks.5.0.conv_dw.weight`, `...se.conv_reduce.bias`, `original_model.bn2.*`),
  `global_pool` and `classifier` replaced by identities as the reference does.  `Encoder.forward(img)` returns the reference's
  16-entry feature list: `[img]`, then the output of every top-level child with the children of `blocks` expanded.  Entry 11 is
  `conv_head`'s RAW output (before bn2 / act2): that is what the reference's decoder reads.
* `EncoderMFMA`: the inference path on MI355X.  BatchNorm (eval) is folded into the convolutions; every 1x1 layer runs on the
  bf16x3 matrix-core kernel (`magnet_conv_mfma_ex`, SiLU in its epilogue for the expand layers, the skip connection as its residual
  input); the stem, the depthwise convolutions and squeeze-excite run on the kernels of csrc/enc_kernels.hip.  Activations are the
  convolution kernel's zero-bordered channel-last split-bf16 planes throughout.
  `EncoderMFMA(model, precision="fp16")` (opt-in; default "bf16x3") stores every activation grid as ONE fp16 plane instead — the stem
  output, the expanded tensor, the depthwise output, the scaled tensor and the block output (the residual stream) — and runs every 1x1
  layer on magnet_conv_mfma_f16e: one matrix instruction per product instead of three, half the bytes per element-wise pass.  The 1x1
  weights are rounded once to fp16 after the fp64 BatchNorm fold; depthwise weights, biases and squeeze-excite stay fp32, and the
  squeeze mean is taken from fp32 values.  The feature list keeps its contract (NCHW fp32 taps).  A reduced-precision mode, outside the
  project's 1e-4 contract: |activation| and |folded weight| <= 65504 — activation stores clamp, a larger folded weight raises at pack
  time — and 39 blocks of 11-bit storage put the taps 1e-3 to 5e-3 of their largest magnitude from fp64
  (profiles/encoder_precision/NOTES.md).
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lib
from .planes import PackCache, fold_bn, pack_taps, pack_taps_f16, plane_f16, planes, round_up, timed

BN_EPS = 1e-3
STEM = 48
HEAD = 2048
# (type, repeats, kernel, stride of the first block, expansion, output channels): tf_efficientnet_b5 (width 1.6, depth 2.2)
STAGES = (("ds", 3, 3, 1, 1, 24), ("ir", 5, 3, 2, 6, 40), ("ir", 5, 5, 2, 6, 64), ("ir", 7, 3, 2, 6, 128),
          ("ir", 7, 5, 1, 6, 176), ("ir", 9, 5, 2, 6, 304), ("ir", 3, 3, 1, 6, 512))
N_FEATURES = 16                                              # [img] + conv_stem, bn1, act1, 7 stages, conv_head, bn2, act2, global_pool, classifier
TAPS = (4, 5, 6, 8, 11)                                      # what the decoder (and the 1/2-scale skip) reads
PRECISIONS = ("bf16x3", "fp16")                              # EncoderMFMA(precision=...): the storage / operand format
F16_MAX = 65504.0                                            # largest finite fp16: the domain of precision="fp16"
PARAMETERS = 28_340_784                                      # 30 389 784 (published B5) - 2 049 000 (the removed classifier)


def same_pad(size: int, k: int, stride: int):
    """TF "SAME" padding of one axis: (before, after).  out = ceil(size / stride), total = max((out - 1) stride + k - size, 0); the
    smaller half goes in front."""
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return total // 2, total - total // 2


class Conv2dSame(nn.Conv2d):
    """nn.Conv2d (no bias) with TF "SAME" padding computed from the input size: asymmetric for stride 2 on an even size."""

    def __init__(self, cin, cout, k, stride=1, groups=1):
        super().__init__(cin, cout, k, stride=stride, padding=0, groups=groups, bias=False)

    def forward(self, x):
        k, s = self.kernel_size[0], self.stride[0]
        (t, b), (l, r) = same_pad(x.shape[2], k, s), same_pad(x.shape[3], k, s)
        if t or b or l or r:
            x = F.pad(x, (l, r, t, b))
        return F.conv2d(x, self.weight, None, self.stride, 0, 1, self.groups)


class SqueezeExcite(nn.Module):
    """x * sigmoid(conv_expand(silu(conv_reduce(mean_hw(x)))))."""

    def __init__(self, chs, reduced):
        super().__init__()
        self.conv_reduce = nn.Conv2d(chs, reduced, 1, bias=True)
        self.act1 = nn.SiLU()
        self.conv_expand = nn.Conv2d(reduced, chs, 1, bias=True)

    def forward(self, x):
        g = self.conv_expand(self.act1(self.conv_reduce(x.mean((2, 3), keepdim=True))))
        return x * torch.sigmoid(g)


class DepthwiseSeparableConv(nn.Module):
    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.has_residual = stride == 1 and cin == cout
        self.conv_dw = Conv2dSame(cin, cin, k, stride, groups=cin)
        self.bn1 = nn.BatchNorm2d(cin, eps=BN_EPS)
        self.act1 = nn.SiLU()
        self.se = SqueezeExcite(cin, int(cin * 0.25))
        self.conv_pw = Conv2dSame(cin, cout, 1)
        self.bn2 = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.act2 = nn.Identity()

    def forward(self, x):
        y = self.se(self.act1(self.bn1(self.conv_dw(x))))
        y = self.act2(self.bn2(self.conv_pw(y)))
        return y + x if self.has_residual else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, k, stride, expansion):
        super().__init__()
        mid = cin * expansion
        self.has_residual = stride == 1 and cin == cout
        self.conv_pw = Conv2dSame(cin, mid, 1)
        self.bn1 = nn.BatchNorm2d(mid, eps=BN_EPS)
        self.act1 = nn.SiLU()
        self.conv_dw = Conv2dSame(mid, mid, k, stride, groups=mid)
        self.bn2 = nn.BatchNorm2d(mid, eps=BN_EPS)
        self.act2 = nn.SiLU()
        self.se = SqueezeExcite(mid, int(cin * 0.25))
        self.conv_pwl = Conv2dSame(mid, cout, 1)
        self.bn3 = nn.BatchNorm2d(cout, eps=BN_EPS)

    def forward(self, x):
        y = self.act1(self.bn1(self.conv_pw(x)))
        y = self.se(self.act2(self.bn2(self.conv_dw(y))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.has_residual else y


class GenEfficientNetB5(nn.Module):
    """The attribute structure of GenEfficientNet for tf_efficientnet_b5, `global_pool` and `classifier` already identities."""

    def __init__(self):
        super().__init__()
        self.conv_stem = Conv2dSame(3, STEM, 3, 2)
        self.bn1 = nn.BatchNorm2d(STEM, eps=BN_EPS)
        self.act1 = nn.SiLU()
        stages, cin = [], STEM
        for kind, repeats, k, stride, expansion, cout in STAGES:
            blocks = []
            for i in range(repeats):
                s = stride if i == 0 else 1
                blocks.append(DepthwiseSeparableConv(cin, cout, k, s) if kind == "ds" else InvertedResidual(cin, cout, k, s, expansion))
                cin = cout
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)
        self.conv_head = Conv2dSame(cin, HEAD, 1)
        self.bn2 = nn.BatchNorm2d(HEAD, eps=BN_EPS)
        self.act2 = nn.SiLU()
        self.global_pool = nn.Identity()
        self.classifier = nn.Identity()

    def forward(self, x):
        x = self.act1(self.bn1(self.conv_stem(x)))
        return self.classifier(self.global_pool(self.act2(self.bn2(self.conv_head(self.blocks(x))))))


def check_precision(precision, who="EncoderMFMA"):
    """`precision` if it is one of PRECISIONS, else MagnetError naming `who`."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise lib.MagnetError(f"{who}: precision must be 'bf16x3' or 'fp16', got {precision!r}")
    return precision


class Encoder(nn.Module):
    """models/submodules/D_dense_depth.py:7-25.  backend: 'torch' (default) runs the modules as they are; 'hip' runs an eval-mode
    forward of a GPU tensor on EncoderMFMA (entries 0, 4, 5, 6, 8, 11 of the list are filled, the others are None: no decoder reads
    them); a .train()-mode forward always runs the torch modules.
    precision: EncoderMFMA's format, 'bf16x3' (default) or 'fp16' (reduced precision, opt-in: see EncoderMFMA); 'fp16' needs
    backend='hip'."""

    def __init__(self, backend: str = "torch", precision: str = "bf16x3"):
        super().__init__()
        if backend not in ("torch", "hip"):
            raise lib.MagnetError(f"Encoder: backend must be 'torch' or 'hip', got {backend!r}")
        self.precision = check_precision(precision, "Encoder")
        if precision == "fp16" and backend != "hip":
            raise lib.MagnetError("Encoder: precision='fp16' is a mode of the HIP path: it needs backend='hip'")
        self.backend = backend
        self.original_model = GenEfficientNetB5()
        self._runner = EncoderMFMA(self.original_model, precision=precision) if backend == "hip" else None

    def forward(self, x):
        if self._runner is not None and not self.training:
            return self._runner.run(x)
        features = [x]
        for k, v in self.original_model._modules.items():
            if k == "blocks":
                for vi in v._modules.values():
                    features.append(vi(features[-1]))
            else:
                features.append(v(features[-1]))
        return features


# ======================================================================================================
# seeded weights
# ======================================================================================================
def _bn_names(model: nn.Module):
    return [n for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)]


def seeded_encoder_state(seed=0):
    """Deterministic weights for `Encoder().state_dict()`: {key: tensor}.  Each key draws from its own generator (seeded by the key's
    CRC32 and `seed`, as dnet.seeded_decoder_state): convolutions He-normal over fan-in, squeeze-excite biases N(0, 0.05^2), BatchNorm
    gamma U(0.6, 1.4), beta N(0, 0.1^2).  Then the seeding is CALIBRATED: one seeded 1 x 3 x 480 x 640 image runs through the torch module
    on the CPU and every BatchNorm's running mean / variance is set to the statistics it saw there, so the activations of the 39 blocks
    stay of order 1 (no blow-up, no collapse to zero) and a parity test of the whole network tests something."""
    enc = Encoder()
    sd = enc.state_dict()
    bn_stems = {"original_model." + n if n else "original_model" for n in _bn_names(enc.original_model)}
    vals = {}
    for key, t in sd.items():
        shape = tuple(t.shape)
        rng = np.random.default_rng([zlib.crc32(key.encode()), int(seed)])
        stem, leaf = key.rsplit(".", 1)
        is_bn = stem in bn_stems
        if leaf == "num_batches_tracked":
            v = np.zeros(shape)
        elif len(shape) == 4:
            v = rng.standard_normal(shape) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif leaf == "running_mean":
            v = np.zeros(shape)
        elif leaf == "running_var":
            v = np.ones(shape)
        elif leaf == "weight" and is_bn:
            v = rng.uniform(0.6, 1.4, shape)
        elif leaf == "bias":
            v = rng.standard_normal(shape) * (0.1 if is_bn else 0.05)
        else:
            raise lib.MagnetError(f"seeded_encoder_state: no rule for {key}")
        vals[key] = torch.from_numpy(np.asarray(v)).to(t.dtype)
    enc.load_state_dict(vals)
    # calibration: momentum 1 makes running_mean / running_var the statistics of this one batch
    bns = [m for m in enc.modules() if isinstance(m, nn.BatchNorm2d)]
    enc.train()
    for m in bns:
        m.momentum = 1.0
    g = torch.Generator().manual_seed(int(seed) + 0x5EED)
    with torch.no_grad():
        enc(torch.rand(1, 3, 480, 640, generator=g))
    out = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    for k in out:
        if k.endswith("num_batches_tracked"):
            out[k].zero_()
    return out


def load_seeded_encoder(encoder: nn.Module, seed=0):
    """Fill an `Encoder` with seeded_encoder_state(seed)."""
    encoder.load_state_dict(seeded_encoder_state(seed))
    return encoder


# ======================================================================================================
# inference on the matrix cores
# ======================================================================================================
# the convolution kernel's output widths (include/magnet_hip.h): a multiple of 128, or 144, 64, 32, 16
def cout_pad_of(c: int) -> int:
    for m in (32, 64, 128, 144):
        if c <= m:
            return m
    return round_up(c, 128)


def blocks_of(model):
    """Every block of a GenEfficientNet in forward order: (name, block, is the depthwise-separable form)."""
    for s, stage in enumerate(model.blocks):
        for b, blk in enumerate(stage):
            yield f"blocks.{s}.{b}", blk, hasattr(blk, "conv_pw") and not hasattr(blk, "conv_pwl")


class EncoderMFMA:
    """Inference runner for a `GenEfficientNetB5` (or a GenEfficientNet instance of the same attribute structure), eval mode.
    precision: 'bf16x3' (default: split-bf16 planes, three matrix instructions per product, fp32-grade) or 'fp16' (ONE fp16 plane per
    activation grid, one matrix instruction per product; reduced precision, |activation| <= 65504 or clamped, a folded 1x1 weight
    beyond 65504 raises when the weights are packed).  Weights and buffers are keyed by precision and live in the runner: two runners
    on one module do not disturb each other."""

    # every launch appends (start_event, end_event, flops, layer name) when set to a list (tools/bench_encoder.py)
    event_sink = None

    def __init__(self, model: nn.Module, precision: str = "bf16x3"):
        self.model = model
        self.precision = check_precision(precision)
        self._packed = None
        self._cache = PackCache(lambda: list(model.parameters()) + list(model.buffers()))
        self._bufs = {}
        self._bufs_sig = None

    # ---- weights ---------------------------------------------------------------------------------------------
    def packed(self, device):
        self._packed = self._cache.get(device, lambda: self._pack(device), self.precision)   # one pack per precision
        return self._packed

    @staticmethod
    def _pw(conv, bn, device, name="", f16=False):
        """A 1x1 layer for the matrix-core kernel: split planes (1, cout_pad, cin_pad), bias (cout_pad), BatchNorm folded in fp64.
        f16: (w, None, bias, cout, slices) with w ONE fp16 plane (1, width, cin_pad), rounded once from the fp32 cast of the fold.
        slices = ((c0, w_slice, bias_slice), ...): the launches of the layer, one per channel slice [c0, c0 + w_slice.shape[1]) of the
        `width`-wide output buffer.  One slice for every width magnet_conv_mfma_f16e serves (32, 64, multiples of 128); the 144
        outputs of stage 1's expand layers are 128 + 32 in a 160-wide buffer (256 lanes would undo the halving on the largest tensor
        of the network)."""
        if bn is None:
            w, b = conv.weight.detach().double(), torch.zeros(conv.out_channels, dtype=torch.float64)
        else:
            w, b = fold_bn(conv, bn)
        cout, cin = w.shape[:2]
        cp = cout_pad_of(cout)
        cuts = (0, cp)
        if f16:
            peak = float(w.float().abs().max().cpu()) if w.numel() else 0.0
            if not peak <= F16_MAX:                                  # an error, never a silent clamp
                raise lib.MagnetError(f"EncoderMFMA {name}: folded weight magnitude {peak:.6g} is outside fp16's range (|w| <= {F16_MAX:.0f}): "
                                      "precision='fp16' cannot hold this encoder; use precision='bf16x3'")
            if cp == 144:
                cp, cuts = 160, (0, 128, 160)
        wf = torch.zeros((cp, round_up(cin, 32), 1, 1), dtype=torch.float32)
        wf[:cout, :cin] = w.float().cpu()
        bias = torch.zeros(cp, dtype=torch.float32)
        bias[:cout] = b.float().cpu()
        if f16:
            wh, bias = pack_taps_f16(wf.to(device)), bias.to(device)
            slices = tuple((c0, wh[:, c0:c1].contiguous(), bias[c0:c1].contiguous()) for c0, c1 in zip(cuts, cuts[1:]))
            return wh, None, bias, cout, slices
        hi, lo = pack_taps(wf.to(device))
        return hi, lo, bias.to(device), cout

    @staticmethod
    def _dw(conv, bn, device):
        """A depthwise layer: folded fp32 weights [k*k][C_pad] (zero in the pad lanes), bias [C_pad], k, stride."""
        w, b = fold_bn(conv, bn)
        C, k = w.shape[0], w.shape[2]
        cp = round_up(C, 32)
        wt = torch.zeros((k * k, cp), dtype=torch.float32)
        wt[:, :C] = w.float().cpu().reshape(C, k * k).t()
        bias = torch.zeros(cp, dtype=torch.float32)
        bias[:C] = b.float().cpu()
        return wt.contiguous().to(device), bias.to(device), k, conv.stride[0], C

    @staticmethod
    def _se(se, device):
        """Squeeze-excite: both weight matrices as (R, C) fp32 (the expand matrix transposed), their biases."""
        C, R = se.conv_reduce.in_channels, se.conv_reduce.out_channels
        f = lambda t: t.detach().float().contiguous().to(device)
        return (f(se.conv_reduce.weight.reshape(R, C)), f(se.conv_reduce.bias), f(se.conv_expand.weight.reshape(C, R).t()),
                f(se.conv_expand.bias), C, R)

    @torch.no_grad()
    def _pack(self, device):
        m = self.model
        P = {}
        w, b = fold_bn(m.conv_stem, m.bn1)
        if tuple(w.shape) != (STEM, 3, 3, 3) or m.conv_stem.stride[0] != 2:
            raise lib.MagnetError("EncoderMFMA: the stem must be a 3x3 stride-2 convolution 3 -> 48")
        P["stem"] = (w.float().reshape(STEM, 27).contiguous().to(device), b.float().contiguous().to(device))
        f16 = self.precision == "fp16"
        for name, blk, ds in blocks_of(m):
            if ds:
                P[name + ".dw"] = self._dw(blk.conv_dw, blk.bn1, device)
                P[name + ".pwl"] = self._pw(blk.conv_pw, blk.bn2, device, name + ".pwl", f16)
            else:
                P[name + ".pw"] = self._pw(blk.conv_pw, blk.bn1, device, name + ".pw", f16)
                P[name + ".dw"] = self._dw(blk.conv_dw, blk.bn2, device)
                P[name + ".pwl"] = self._pw(blk.conv_pwl, blk.bn3, device, name + ".pwl", f16)
            P[name + ".se"] = self._se(blk.se, device)
        P["conv_head"] = self._pw(m.conv_head, None, device, "conv_head", f16)
        return P

    # ---- activations -----------------------------------------------------------------------------------------
    def _grid(self, tag, dev, N, h, w, c):
        """A zero-bordered (N, h+2, w+2, c) grid as a (hi, lo) pair of (rows, c) planes, zero at allocation (border and pad lanes stay zero:
        no launch writes them with anything else).  precision='fp16': (ONE fp16 plane, None)."""
        key = (tag, h, w, c)
        b = self._bufs.get(key)
        if b is None:
            rows = N * (h + 2) * (w + 2)
            b = self._bufs[key] = (plane_f16(rows, c, dev, zero=True), None) if self.precision == "fp16" else planes(rows, c, dev, zero=True)
        return b

    def _scratch(self, tag, dev, shape):
        key = (tag,) + tuple(shape)
        b = self._bufs.get(key)
        if b is None:
            b = self._bufs[key] = torch.empty(shape, dtype=torch.float32, device=dev)
        return b

    def _conv(self, name, src, in_ld, N, h, w, dst=None, out_ld=0, silu=False, add=None, out_f32=None):
        hi, lo, bias, cout = self._packed[name][:4]
        rows, cin = N * (h + 2) * (w + 2), hi.shape[2]
        if self.precision == "fp16":                                # one launch per channel slice of the layer (one, but for 144 outputs)
            for c0, ws, bs in self._packed[name][4]:
                with timed(EncoderMFMA.event_sink, 2.0 * rows * cin * ws.shape[1], name):
                    lib.conv_mfma(src[0], None, in_ld, cin, ws, None, bs, 1, w + 2, False, rows, out_hi=None if dst is None else dst[0][:, c0:],
                                  out_f32=None if out_f32 is None else out_f32[..., c0:], out_ld=out_ld or hi.shape[1],
                                  add=None if add is None else (add[0][:, c0:], None, add[2]), border=(h + 2, 1),
                                  repad=1 if out_f32 is not None else 0, silu=silu, f16="enc")
            return
        with timed(EncoderMFMA.event_sink, 2.0 * rows * cin * hi.shape[1], name):
            lib.conv_mfma(src[0], src[1], in_ld, cin, hi, lo, bias, 1, w + 2, False, rows,
                          out_hi=None if dst is None else dst[0], out_lo=None if dst is None else dst[1], out_f32=out_f32,
                          out_ld=out_ld, add=add, border=(h + 2, 1), repad=1 if out_f32 is not None else 0, silu=silu)

    def _dw_se(self, name, src, N, h, w, dev):
        """Depthwise convolution + folded BatchNorm + SiLU of grid `src` (N, h+2, w+2, C_pad), then squeeze-excite in place: returns
        (planes, ho, wo)."""
        wt, bias, k, stride, C = self._packed[name + ".dw"]
        cp = wt.shape[1]
        (pt, _), (pl, _) = same_pad(h, k, stride), same_pad(w, k, stride)
        ho, wo = -(-h // stride), -(-w // stride)
        dst = self._grid("D", dev, N, ho, wo, cp)
        n_part = lib.dwconv_parts(ho, wo)
        part = self._scratch("part", dev, (N, n_part, cp))
        sink = EncoderMFMA.event_sink
        f16 = self.precision == "fp16"
        with timed(sink, 2.0 * N * ho * wo * C * k * k, name + ".dw"):
            if f16:
                lib.dwconv_cl_f16(src[0], src[0].shape[1], N, h, w, cp, wt, bias, k, stride, pt, pl, dst[0], cp, part)
            else:
                lib.dwconv_cl(src[0], src[1], src[0].shape[1], N, h, w, cp, wt, bias, k, stride, pt, pl, dst[0], dst[1], cp, part)
        w1, b1, w2t, b2, C, R = self._packed[name + ".se"]
        gate = self._scratch("gate", dev, (N, cp))
        with timed(sink, 4.0 * N * C * R, name + ".se_gate"):
            lib.se_gate(part, n_part, ho * wo, w1, b1, w2t, b2, C, R, gate)
        with timed(sink, 1.0 * N * ho * wo * C, name + ".se_scale"):
            if f16:
                lib.se_scale_f16(dst[0], cp, gate, N, ho, wo, cp, dst[0], cp)
            else:
                lib.se_scale(dst[0], dst[1], cp, gate, N, ho, wo, cp, dst[0], dst[1], cp)
        return dst, ho, wo

    @staticmethod
    def _nchw(buf, N, h, w, C):
        """The interior of a grid as an NCHW fp32 tensor (an fp16 plane: a slice, then .float())."""
        if buf[1] is None:
            return buf[0].view(N, h + 2, w + 2, -1)[:, 1:h + 1, 1:w + 1, :C].float().permute(0, 3, 1, 2).contiguous()
        hi, lo = (t.view(N, h + 2, w + 2, -1)[:, 1:h + 1, 1:w + 1, :C] for t in buf)
        return (hi.float() + lo.float()).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def run(self, img: torch.Tensor):
        """img (N,3,H,W) fp32 on the GPU -> the 16-entry feature list with NCHW fp32 tensors at [4], [5], [6], [8], [11], `img` at [0]
        and None elsewhere."""
        if not isinstance(img, torch.Tensor) or not img.is_cuda:
            raise lib.MagnetError("EncoderMFMA: image must be on the GPU (no CPU fallback)")
        if self.model.training:
            raise lib.MagnetError("EncoderMFMA folds BatchNorm running statistics: call .eval() on the encoder first")
        if img.dim() != 4 or img.shape[1] != 3:
            raise lib.MagnetError(f"EncoderMFMA: image must be (N, 3, H, W), got {tuple(img.shape)}")
        x_img = img.detach().float().contiguous()
        N, _, H, W = x_img.shape
        dev = x_img.device
        P = self.packed(dev)
        sig = (str(dev), N, H, W, self.precision)
        if self._bufs_sig != sig:                                   # one batch shape at a time
            self._bufs.clear()
            self._bufs_sig = sig
        feats = [img] + [None] * (N_FEATURES - 1)
        h, w = -(-H // 2), -(-W // 2)
        x = self._grid("X0", dev, N, h, w, 64)
        with timed(EncoderMFMA.event_sink, 2.0 * N * h * w * 27 * STEM, "stem"):
            if self.precision == "fp16":
                lib.enc_stem_f16(x_img, P["stem"][0], P["stem"][1], x[0])
            else:
                lib.enc_stem(x_img, P["stem"][0], P["stem"][1], x[0], x[1])
        x_ld, flip = 64, 0
        for name, blk, ds in blocks_of(self.model):
            s = int(name.split(".")[1])
            if ds:
                y, ho, wo = self._dw_se(name, x, N, h, w, dev)
            else:
                mid = P[name + ".pw"][0].shape[1]                   # cout_pad of the expand layer; its buffer is a multiple of 32 wide
                e = self._grid("E", dev, N, h, w, round_up(mid, 32))
                self._conv(name + ".pw", x, x_ld, N, h, w, dst=e, out_ld=e[0].shape[1], silu=True)
                y, ho, wo = self._dw_se(name, e, N, h, w, dev)
            cp = P[name + ".pwl"][0].shape[1]
            flip ^= 1
            out = self._grid(f"X{flip}", dev, N, ho, wo, cp)
            add = (x[0], x[1], x_ld) if blk.has_residual else None
            self._conv(name + ".pwl", y, y[0].shape[1], N, ho, wo, dst=out, add=add)
            x, x_ld, h, w = out, cp, ho, wo
            if s + 4 in TAPS and name == f"blocks.{s}.{len(self.model.blocks[s]) - 1}":     # the stage's output is a tap
                feats[s + 4] = self._nchw(x, N, h, w, P[name + ".pwl"][3])
        head = self._scratch("head", dev, (N, h, w, P["conv_head"][0].shape[1]))
        self._conv("conv_head", x, x_ld, N, h, w, out_f32=head)
        feats[11] = head.permute(0, 3, 1, 2).contiguous()
        return feats

    def __call__(self, img):
        return self.run(img)
