"""D-Net (MaGNet's single-view depth network): the DenseDepth_BN decoder of the reference at downsample ratio 4
(models/DNET.py, models/submodules/D_dense_depth.py:28-43,104-195) — by arithmetic the largest block of end-to-end inference
(about 228 GFLOP per 480x640 image).

Three things live here:

* `DenseDepthDecoder` / `DNET`: plain nn.Modules with the reference's architecture and **state_dict keys** (`conv2.*`,
  `up1._net.{0,1,3,4}.*`, ..., `depth_head.{0,2,4}.*`, `mask_head.{0,2,4}.*`; `d_net.encoder.*` / `d_net.decoder.*` under DNET), so a
  reference D-Net checkpoint loads unchanged.  The encoder (EfficientNet-B5 through torch.hub in the reference) is the caller's module:
  anything that maps images to the reference's feature list (the decoder reads indices 5, 6, 8 and 11).
* `seeded_decoder_state`: a deterministic numpy weight recipe per state_dict key (He-normal convolutions, non-trivial BatchNorm
  statistics) shared by the golden generator (tests/golden/make_golden_dnet.py), the tests and the benchmark.
* `DNetMFMA`: the decoder's inference path on MI355X.  BatchNorm (eval) is folded into the convolutions in fp64 on the host; every
  convolution runs on the bf16x3 matrix-core kernel (fp32-grade) with LeakyReLU in its epilogue (magnet_conv_mfma_ex); activations are
  zero-bordered channel-last split-bf16 planes; the bilinear upsampling and the skip features land in channel slices of the next
  block's input (magnet_upsample_bilinear_cl, magnet_pack_split); the depth head runs as one fused launch and the Gaussian activation
  behind it is csrc/dnet_kernels.hip.  `run(..., x_d3_out=...)` writes the reference frames' x_feat straight into MAGNET's G-Net input
  buffer (interior rows, zero border, a channel slice): no NCHW x_d3, no repack.  `run_standalone` is the stand-alone D-Net
  (`DNET(dnet=True)`, what test_DNet.py evaluates): the same decoder pass, then the depth head and the mask head as two fused launches
  and magnet_dnet_upsample_gauss (learned convex upsampling x4 of the raw (mu, v), activation_G behind it) -> (N, 2, H, W)
  [mu, variance].  `DNET(..., backend="hip")` routes an eval-mode forward through it.
  `DNetMFMA(decoder, split_k="auto")` (opt-in; default 0 = off) runs conv2 and up1.0 .. up3.1 as split-K launches
  (magnet_conv_mfma_splitk) where a launch has too few tiles to fill the chip — one to a few images; `split_factor` is the rule.
  Under "auto" the factor S of a launch depends on its tile count, so the bits of one image can differ between batch sizes — by the
  order of S - 1 fp32 additions per output only; with a forced dict {layer: S} they do not.  SequenceRunner's bit-equality with
  MAGNET.forward holds when both ran the same factors.
  `DNetMFMA(decoder, precision="fp16")` (opt-in; default "bf16x3") runs conv2 and up1.0 .. up3.1 on the single-plane fp16 format
  (magnet_conv_mfma_f16d, one matrix instruction per product instead of three): the folded weights are rounded once to fp16, every
  activation buffer between conv2 and up3's second convolution is ONE zero-bordered fp16 plane (magnet_pack_f16,
  magnet_upsample_bilinear_cl_f16, out_mode 3), the compact hand-overs to the bilinear upsampling stay fp32 and x_feat leaves as the
  split-bf16 planes (or NCHW fp32) of the default mode, so the heads, G-Net and SequenceRunner see today's formats.  A reduced-precision
  mode: |activation| and |folded weight| <= 65504 — activation stores clamp (NaN passes through), a larger folded weight raises at
  pack time; relative rounding 2^-11 per stored value.  It composes with split_k (magnet_conv_mfma_f16d_splitk).  Measured in
  profiles/dnet_precision/NOTES.md.
"""
from __future__ import annotations

import contextlib
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lib
from .convnet import ConvStackMFMA
from .planes import PackCache, fold_bn, pack_taps, pack_taps_f16, plane_f16, planes, round_up, timed

# (block, skip feature index, skip channels, output channels) at downsample ratio 4 (D_dense_depth.py:130-135,176-180)
_UP = (("up1", 8, 176, 1024), ("up2", 6, 64, 512), ("up3", 5, 40, 256))
_SKIP_IN = 11                                              # x_block4: 2048 channels at 1/32 (the input of conv2)
SPLIT_LAYERS = ("conv2", "up1.0", "up1.1", "up2.0", "up2.1", "up3.0", "up3.1")    # the launches DNetMFMA(split_k=...) covers
# constants of the "auto" rule (split_factor), from the sweep in profiles/splitk/NOTES.md
SPLIT_CUS = 256                                            # a launch with a workgroup per CU is not split; a split fills at most one per CU ...
SPLIT_SLOTS = 512                                          # ... or, from half the CUs on, the resident slots (two 4-wave workgroups per CU)
PRECISIONS = ("bf16x3", "fp16")                            # DNetMFMA(precision=...): the decoder's operand format
F16_MAX = 65504.0                                          # largest finite fp16: the domain of precision="fp16"
SPLIT_AUTO_MIN_CHUNKS = 4                                  # 32-channel chunks per split under "auto" (>= lib.SPLITK_MIN_CHUNKS): the
                                                           # shortest split the sweep still saw pay (up2.1 at S = 4)


def split_factor(row_tiles, n_tiles, cin_chunks):
    """The "auto" split-K factor of a plain decoder launch of row_tiles x n_tiles workgroups (128 rows x 128 channels each) whose input has
    cin_chunks 32-channel chunks.  1 (no split) when the launch already has a workgroup per CU (SPLIT_CUS).  Below that, the largest S
    that keeps ONE workgroup per CU (workgroups x S <= SPLIT_CUS) — measured faster than filling the second resident slot of a CU:
    88 workgroups at K = 20 160 take 0.40 ms unsplit, 0.23 ms at S = 2 (176 workgroups) and 0.27 ms at S = 5 (440) — and S = 2 where
    even that overfills the CUs (more than SPLIT_CUS / 2 workgroups; the split stays within SPLIT_SLOTS).  Never more than
    lib.SPLITK_MAX, never fewer than SPLIT_AUTO_MIN_CHUNKS chunks per split.  Pure host arithmetic; non-increasing in the workgroup
    count."""
    wg = int(row_tiles) * int(n_tiles)
    if wg <= 0 or cin_chunks <= 0:
        raise lib.MagnetError(f"split_factor: row_tiles={row_tiles} n_tiles={n_tiles} cin_chunks={cin_chunks} must be positive")
    if wg >= SPLIT_CUS:
        return 1
    s = SPLIT_CUS // wg
    if s < 2:
        s = min(2, SPLIT_SLOTS // wg)
    s = min(s, lib.SPLITK_MAX, int(cin_chunks) // max(SPLIT_AUTO_MIN_CHUNKS, lib.SPLITK_MIN_CHUNKS))
    return s if s >= 2 else 1


def check_precision(precision, who="DNetMFMA", what="precision"):
    """'bf16x3' or 'fp16'; MagnetError otherwise."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise lib.MagnetError(f"{who}: {what} must be 'bf16x3' or 'fp16', got {precision!r}")
    return precision


def check_split_k(split_k, who="DNetMFMA"):
    """0 (off), "auto" or {layer name: S} with S in 1 .. lib.SPLITK_MAX (1 = that layer unsplit); MagnetError otherwise."""
    if isinstance(split_k, dict):
        for k, v in split_k.items():
            if k not in SPLIT_LAYERS or isinstance(v, bool) or not isinstance(v, int) or not (1 <= v <= lib.SPLITK_MAX):
                raise lib.MagnetError(f"{who}: split_k[{k!r}] = {v!r}: layers are {SPLIT_LAYERS}, factors 1 .. {lib.SPLITK_MAX}")
        return dict(split_k)
    if split_k == "auto" or (split_k == 0 and isinstance(split_k, int) and not isinstance(split_k, bool)):
        return split_k
    raise lib.MagnetError(f"{who}: split_k must be 0 (off), 'auto' or a dict {{layer: S}}, got {split_k!r}")


class UpSampleBN(nn.Module):
    """Bilinear (align_corners=True) to the skip tensor's size, concatenate [up, skip], then twice conv3x3-BN-LeakyReLU
    (D_dense_depth.py:28-43)."""

    def __init__(self, skip_input, output_features):
        super().__init__()
        self._net = nn.Sequential(nn.Conv2d(skip_input, output_features, 3, padding=1), nn.BatchNorm2d(output_features), nn.LeakyReLU(),
                                  nn.Conv2d(output_features, output_features, 3, padding=1), nn.BatchNorm2d(output_features),
                                  nn.LeakyReLU())

    def forward(self, x, concat_with):
        up = F.interpolate(x, size=[concat_with.size(2), concat_with.size(3)], mode="bilinear", align_corners=True)
        return self._net(torch.cat([up, concat_with], dim=1))


def _head(cin, h_dim, cout):
    return nn.Sequential(nn.Conv2d(cin, h_dim, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(h_dim, h_dim, 1), nn.ReLU(inplace=True),
                         nn.Conv2d(h_dim, cout, 1))


def upsample_depth_via_mask(depth, up_mask, k):
    """Learned convex upsampling of the stand-alone D-Net (D_dense_depth.py:72-88)."""
    N, C, H, W = depth.shape
    wgt = torch.softmax(up_mask.reshape(N, 1, 9, k, k, H, W), dim=2)
    patch = F.unfold(depth, [3, 3], padding=1).reshape(N, C, 9, 1, 1, H, W)
    return (wgt * patch).sum(dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, C, k * H, k * W)


class DenseDepthDecoder(nn.Module):
    """The reference's `Decoder(num_classes, downsample_ratio=4, learned_upsampling=True, BN=True, dnet)`.
    dnet=False (MaGNet): forward(features) -> (depth head output (N, num_classes, H/4, W/4), x_feat (N, 256, H/4, W/4));
    dnet=True (stand-alone D-Net): the depth upsampled x4 through the learned mask head, or with forward(features, upsample=False) the
    raw pair (depth (N, num_classes, H/4, W/4), up_mask (N, 144, H/4, W/4)) for losses.DnetLoss."""

    def __init__(self, num_classes=2, downsample_ratio=4, dnet=False):
        super().__init__()
        if downsample_ratio != 4:
            raise lib.MagnetError(f"DenseDepthDecoder: downsample_ratio {downsample_ratio} is not built (MaGNet uses 4)")
        features = 2048
        self.downsample_ratio = downsample_ratio
        self.dnet = dnet
        self.conv2 = nn.Conv2d(features, features, 1)
        self.up1 = UpSampleBN(features + 176, features // 2)
        self.up2 = UpSampleBN(features // 2 + 64, features // 4)
        self.up3 = UpSampleBN(features // 4 + 40, features // 8)
        self.depth_head = _head(features // 8, 128, num_classes)
        self.mask_head = _head(features // 8, 128, 9 * downsample_ratio * downsample_ratio)

    def forward(self, features, upsample=True):
        x_d0 = self.conv2(features[_SKIP_IN])
        x_d1 = self.up1(x_d0, features[8])
        x_d2 = self.up2(x_d1, features[6])
        x_feat = self.up3(x_d2, features[5])
        depth = self.depth_head(x_feat)
        if not upsample and not self.dnet:
            raise lib.MagnetError("DenseDepthDecoder: upsample=False is the stand-alone D-Net's form (dnet=True)")
        if self.dnet:
            if not upsample:                                       # the raw pair that losses.DnetLoss fuses with the loss
                return depth, self.mask_head(x_feat)
            return upsample_depth_via_mask(depth, self.mask_head(x_feat), self.downsample_ratio)
        return depth, x_feat


class DenseDepth(nn.Module):
    """encoder (the caller's module: img -> feature list) + DenseDepthDecoder (D_dense_depth.py:198-213)."""

    def __init__(self, encoder, num_classes=2, downsample_ratio=4, dnet=False):
        super().__init__()
        self.encoder = encoder
        self.decoder = DenseDepthDecoder(num_classes, downsample_ratio, dnet)

    def forward(self, x, upsample=True):
        feats = self.encoder(x)
        return self.decoder(feats) if upsample else self.decoder(feats, upsample=False)


def gaussian_activation(out, magnet=True):
    """activation_G_magnet (models/DNET.py:62-67; magnet=True): (mu, sigma = sqrt(elu(v) + 1 + 1e-10)) of the head output, x_feat
    passed through.  magnet=False: activation_G (DNET.py:55-60), the stand-alone D-Net's (mu, variance)."""
    if not magnet:
        mu, var = torch.split(out, 1, dim=1)
        return torch.cat([mu, F.elu(var) + 1.0 + 1e-10], dim=1)
    mu, var = torch.split(out[0], 1, dim=1)
    var = F.elu(var) + 1.0 + 1e-10
    return torch.cat([mu, torch.sqrt(var)], dim=1), out[1]


class DNET(nn.Module):
    """models/DNET.py with output_type 'G' and DNET_architecture 'DenseDepth_BN': `DNET(args, encoder, dnet=False)` is MaGNet's
    D-Net, img -> ((N, 2, H/4, W/4) [mu, sigma], x_feat (N, 256, H/4, W/4)); `dnet=True` is the stand-alone D-Net of test_DNet.py /
    train_DNet.py, img -> (N, 2, H, W) [mu, variance], or with forward(img, upsample=False) the raw (depth, up_mask) of the torch modules
    for losses.DnetLoss's fused tail.  `encoder`: any module returning the reference's feature list
    (EfficientNet-B5's, or magnet_amd.standin.StandinEncoder).
    backend: 'torch' (default) runs the modules as they are; 'hip' runs the decoder, the heads and the tail of an eval-mode forward on
    DNetMFMA (the caller's encoder stays a torch module); in .train() the torch forward runs, as MAGNET does for its D-Net.
    split_k: DNetMFMA's split-K mode (0 = off, "auto", or {layer: S}); needs backend='hip'.
    precision: DNetMFMA's operand format, 'bf16x3' (default) or 'fp16' (reduced precision, opt-in: see DNetMFMA); 'fp16' needs
    backend='hip'; in .train() the torch forward runs whatever the value."""

    def __init__(self, args, encoder: nn.Module, dnet: bool = False, backend: str = "torch", split_k=0, precision: str = "bf16x3"):
        super().__init__()
        self.args = args
        if getattr(args, "output_type", "G") != "G":
            raise lib.MagnetError(f"DNET: output_type {args.output_type!r} is not built (MaGNet uses 'G')")
        if getattr(args, "DNET_architecture", "DenseDepth_BN") != "DenseDepth_BN":
            raise lib.MagnetError(f"DNET: architecture {args.DNET_architecture!r} is not built (the BatchNorm decoder 'DenseDepth_BN' is)")
        if backend not in ("torch", "hip"):
            raise lib.MagnetError(f"DNET: backend must be 'torch' or 'hip', got {backend!r}")
        self.dnet = dnet
        self.backend = backend
        self.d_net = DenseDepth(encoder, getattr(args, "output_dim", 2), args.downsample_ratio, dnet)
        self._runner = None
        split_k = check_split_k(split_k, "DNET")
        if split_k != 0 and backend != "hip":
            raise lib.MagnetError("DNET: split_k is a mode of the HIP decoder path: it needs backend='hip'")
        self.precision = check_precision(precision, "DNET")
        if precision == "fp16" and backend != "hip":
            raise lib.MagnetError("DNET: precision='fp16' is a mode of the HIP decoder path: it needs backend='hip'")
        if backend == "hip":
            check_decoder(self.d_net.decoder, standalone=dnet)
            self._runner = DNetMFMA(self.d_net.decoder, split_k=split_k, precision=precision)

    def forward(self, img, upsample=True):
        if not upsample:
            # the training form for losses.DnetLoss: the torch modules up to the two heads, on either backend; the upsampling, the
            # activation and the loss follow fused, so the pair is returned raw: (depth (N,2,h,w) [mu, v], up_mask (N,144,h,w))
            if not self.dnet:
                raise lib.MagnetError("DNET: upsample=False is the stand-alone D-Net's form (dnet=True)")
            return self.d_net(img, upsample=False)
        if self._runner is not None and not self.training:
            feats = self.d_net.encoder(img)
            return self._runner.run_standalone(feats) if self.dnet else self._runner.run(feats)
        return gaussian_activation(self.d_net(img), magnet=not self.dnet)


def seeded_decoder_state(keys_shapes: dict, seed=0):
    """Deterministic weights for a decoder state_dict: {key: np.float64 array}.  `keys_shapes`: {key: shape}, e.g.
    {k: tuple(v.shape) for k, v in decoder.state_dict().items()}.  Each key draws from its own generator (seeded by the key's CRC32
    and `seed`), so the recipe does not depend on key order.  Convolutions He-normal over fan-in with N(0, 0.05^2) biases; BatchNorm
    gamma U(0.6, 1.4), beta N(0, 0.1^2), running mean N(0, 0.2^2), running variance U(0.5, 2): activations neither vanish nor blow up."""
    out = {}
    for key, shape in keys_shapes.items():
        shape = tuple(shape)
        rng = np.random.default_rng([zlib.crc32(key.encode()), int(seed)])
        stem, leaf = key.rsplit(".", 1)
        is_bn = stem + ".running_mean" in keys_shapes
        if leaf == "num_batches_tracked":
            out[key] = np.zeros(shape)
        elif len(shape) == 4:                                              # convolution weight
            out[key] = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif leaf == "running_mean":
            out[key] = rng.standard_normal(shape) * 0.2
        elif leaf == "running_var":
            out[key] = rng.uniform(0.5, 2.0, shape)
        elif leaf == "weight" and is_bn:
            out[key] = rng.uniform(0.6, 1.4, shape)
        elif leaf == "bias":
            out[key] = rng.standard_normal(shape) * (0.1 if is_bn else 0.05)
        else:
            raise lib.MagnetError(f"seeded_decoder_state: no rule for {key}")
    return out


def load_seeded_decoder(decoder: nn.Module, seed=0):
    """Fill `decoder` (ours or the reference's Decoder) with seeded_decoder_state."""
    sd = decoder.state_dict()
    vals = seeded_decoder_state({k: tuple(v.shape) for k, v in sd.items()}, seed)
    decoder.load_state_dict({k: torch.from_numpy(vals[k]).to(sd[k].dtype) for k in sd})
    return decoder


# ======================================================================================================
# inference on the matrix cores
# ======================================================================================================
def check_decoder(decoder: nn.Module, standalone: bool = False):
    """MagnetError unless `decoder` is the reference's BatchNorm decoder at downsample ratio 4 (ours or the reference's class).
    standalone: also require the learned-upsampling mask head (3x3 256->128, 1x1 128->128, 1x1 128->144) of the stand-alone form."""
    if getattr(decoder, "downsample_ratio", None) != 4 or not all(hasattr(decoder, a) for a in ("conv2", "up1", "up2", "up3", "depth_head")):
        raise lib.MagnetError("the HIP D-Net runs the DenseDepth decoder at downsample_ratio 4 (conv2, up1..up3, depth_head)")
    for name, _, _, _ in _UP:
        net = getattr(decoder, name)._net
        if not (isinstance(net[1], nn.BatchNorm2d) and isinstance(net[4], nn.BatchNorm2d) and isinstance(net[2], nn.LeakyReLU)
                and isinstance(net[5], nn.LeakyReLU)):
            raise lib.MagnetError(f"the HIP D-Net runs the BatchNorm decoder (DenseDepth_BN); {name} is not conv-BN-LeakyReLU")
        if type(net[0]) is not nn.Conv2d or type(net[3]) is not nn.Conv2d:
            raise lib.MagnetError(f"the HIP D-Net needs plain nn.Conv2d layers ({name} has weight-standardised convolutions)")
    dh = decoder.depth_head
    if len(dh) != 5 or dh[4].out_channels != 2:
        raise lib.MagnetError("the HIP D-Net needs the 2-output depth head (output_dim 2, output_type 'G')")
    if standalone:
        mh = getattr(decoder, "mask_head", None)
        ok = isinstance(mh, nn.Sequential) and len(mh) == 5 and all(type(mh[i]) is nn.Conv2d for i in (0, 2, 4)) \
            and all(isinstance(mh[i], nn.ReLU) for i in (1, 3))
        ok = ok and (mh[0].in_channels, mh[0].out_channels, mh[0].kernel_size) == (256, 128, (3, 3)) \
            and (mh[2].in_channels, mh[2].out_channels, mh[2].kernel_size) == (128, 128, (1, 1)) \
            and (mh[4].in_channels, mh[4].out_channels, mh[4].kernel_size) == (128, 144, (1, 1))
        if not ok:
            raise lib.MagnetError("the stand-alone HIP D-Net needs the learned-upsampling mask head (3x3 256->128, 1x1 128->128, "
                                  "1x1 128->144: 9 taps x 4 x 4 sub-pixels)")


class DNetMFMA:
    """Inference runner for a DenseDepth_BN decoder at downsample ratio 4 (ours or the reference's `Decoder`), eval mode."""

    # every convolution launch appends (start_event, end_event, flops) when set to a list (tools/bench_dnet.py)
    event_sink = None

    def __init__(self, decoder: nn.Module, split_k=0, precision: str = "bf16x3"):
        """precision: 'bf16x3' (default: split-bf16 planes, three matrix instructions per product, fp32-grade) or 'fp16' (conv2 and
        up1.0 .. up3.1 on one fp16 plane per buffer, one matrix instruction per product; reduced precision, |activation| <= 65504 or
        clamped, a folded weight beyond 65504 raises when the weights are packed)."""
        check_decoder(decoder)
        self.decoder = decoder
        self.precision = check_precision(precision)
        self.launch_log = []                                        # (layer, entry point) of every convolution launch of the last run
        self.split_k = check_split_k(split_k)                       # 0 = off (default), "auto" = split_factor per launch, {layer: S} = forced
        self.factors_used = []                                      # (layer, rows, S) of every covered launch of the last run
        self.slope = float(decoder.up1._net[2].negative_slope)
        dh = decoder.depth_head
        # the depth head (3x3 256->128 ReLU, 1x1 128->128 ReLU, 1x1 128->2) on the stack runner's fused epilogue, which has two hidden
        # 1x1 layers: the second is the identity (its input is non-negative, so the ReLU behind it changes nothing)
        eye = nn.Conv2d(128, 128, 1)
        with torch.no_grad():
            eye.weight.copy_(torch.eye(128).view(128, 128, 1, 1)); eye.bias.zero_()
        self._head = ConvStackMFMA(nn.Sequential(dh[0], nn.ReLU(), dh[2], nn.ReLU(), eye, nn.ReLU(), dh[4]))
        self._head.small_tiles = False                              # the D-Net's own launches keep their 128-row tiles (not measured at one frame)
        self._eye = eye
        self._mask = None                                           # the mask head's stack: built by the first run_standalone()
        self._mask_work = {}
        self._packed = None
        self._cache = PackCache(lambda: list(decoder.parameters()) + list(decoder.buffers()))
        self._bufs = {}
        self._bufs_sig = None
        self._head_work = {}

    def packed(self, device):
        self._packed = self._cache.get(device, lambda: self._pack(device), self.precision)   # one pack per precision
        return self._packed

    @torch.no_grad()
    def _pack(self, device):
        d = self.decoder
        P = {}

        f16 = self.precision == "fp16"

        def put(name, w, b, cin_pad):
            if f16:
                # the fp64 fold, cast to fp32, rounded ONCE to fp16; a weight outside fp16's range is an error, never a silent clamp.
                # The check runs on a host copy of the folded weights (a decoder that lives on the GPU is copied once per pack)
                wf = w.float()
                peak = float(wf.detach().abs().max().cpu()) if wf.numel() else 0.0
                if not peak <= F16_MAX:
                    raise lib.MagnetError(f"DNetMFMA {name}: folded weight magnitude {peak:.6g} is outside fp16's range (|w| <= {F16_MAX:.0f}): "
                                          "precision='fp16' cannot hold this decoder; use precision='bf16x3'")
                hi, lo = pack_taps_f16(wf.to(device), cin_pad), None
            else:
                hi, lo = pack_taps(w.to(device), cin_pad)
            P[name] = (hi, lo, b.float().to(device).contiguous(), hi.shape[0], cin_pad)

        put("conv2", d.conv2.weight.detach().double(), d.conv2.bias.detach().double(), 2048)
        cin = 2048
        for name, _, skip_c, cout in _UP:
            net = getattr(d, name)._net
            put(name + ".0", *fold_bn(net[0], net[1]), round_up(cin + skip_c, 32))
            put(name + ".1", *fold_bn(net[3], net[4]), cout)
            cin = cout
        return P

    def _conv(self, name, src, in_ld, wp, rows, dst=None, out_f32=None, out_ld=0, border=None, repad=0):
        hi, lo, bias, taps, cin = self._packed[name]
        cout = hi.shape[1]
        # every operand must hold what the launch touches (planes may be row / channel views of wider buffers)
        f16 = self.precision == "fp16"
        if f16:                                                     # ONE fp16 plane where the default mode has a (hi, lo) pair
            src = (src,)
            if dst is not None and not isinstance(dst, tuple):
                dst = (dst,)
        for t in src:
            if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) != in_ld or t.shape[0] < rows or t.shape[1] < cin:
                raise lib.MagnetError(f"DNetMFMA {name}: input view {tuple(t.shape)} / pitch {t.stride(0)} does not hold {rows} x {cin} at {in_ld}")
        ld = out_ld or cout
        n_out = rows if not repad else rows // (border[0] * wp) * (border[0] - 2) * (wp - 2)
        for t in (dst if dst is not None else (out_f32,)):
            if t.dim() == 2:
                ok = t.stride(1) == 1 and t.stride(0) == ld and t.shape[0] >= n_out and t.shape[1] >= cout
            else:
                ok = t.is_contiguous() and ld == cout and t.numel() >= n_out * ld
            if not ok:
                raise lib.MagnetError(f"DNetMFMA {name}: output {tuple(t.shape)} does not hold {n_out} rows of {cout} at pitch {ld}")
        S = 1
        if isinstance(self.split_k, dict):
            S = self.split_k.get(name, 1)
        elif self.split_k == "auto":
            S = split_factor((rows + 127) // 128, cout // 128, cin // 32)
        self.factors_used.append((name, rows, S))
        work = None
        if S > 1:
            # one workspace for all launches (stream-ordered: a layer's reduce has read it before the next layer's partials are written),
            # kept with the per-shape buffers and grown on demand
            need = lib.conv_mfma_splitk_workspace(rows, cin, cout, taps, S, f16="wide" if f16 else False) // 4
            work = self._bufs.get("splitk.work")
            if work is None or work.numel() < need:
                work = self._bufs["splitk.work"] = torch.empty(need, dtype=torch.float32, device=src[0].device)
        leaky = None if name == "conv2" else self.slope
        with self._logged(name), timed(DNetMFMA.event_sink, 2.0 * rows * cin * taps * cout):
            if f16:
                # dst of one plane: the fp16 plane (out_mode 3); of two: the split-bf16 pair (out_mode 0: x_feat)
                lib.conv_mfma(src[0], None, in_ld, cin, hi, None, bias, taps, wp, False, rows,
                              out_hi=None if dst is None else dst[0], out_lo=None if dst is None or len(dst) == 1 else dst[1], out_f32=out_f32,
                              out_ld=out_ld, border=border, repad=repad, leaky=leaky, f16="wide", split_k=S if S > 1 else None, work=work)
            else:
                lib.conv_mfma(src[0], src[1], in_ld, cin, hi, lo, bias, taps, wp, False, rows,
                              out_hi=None if dst is None else dst[0], out_lo=None if dst is None else dst[1], out_f32=out_f32, out_ld=out_ld,
                              border=border, repad=repad, leaky=leaky,
                              split_k=S if S > 1 else None, work=work)

    @contextlib.contextmanager
    def _logged(self, layer):
        """The convolution entry points lib calls inside the block are appended to launch_log as (layer, entry point)."""
        prev, lib.entry_log = lib.entry_log, []
        try:
            yield
        finally:
            got, lib.entry_log = lib.entry_log, prev
            self.launch_log += [(layer, e) for e in got if e.startswith("magnet_conv_mfma")]
            if prev is not None:
                prev += got

    def _buffers(self, dev, N, dims):
        sig = (str(dev), N, dims, self.precision)
        if self._bufs_sig == sig:
            return self._bufs
        self._bufs.clear()                                          # one shape at a time: the buffers are large
        self._head_work.clear()
        self._mask_work.clear()
        self._bufs_sig = sig
        (h32, w32), (h16, w16), (h8, w8), (h4, w4) = dims
        r = lambda h, w: N * (h + 2) * (w + 2)
        b = self._bufs
        # precision="fp16": ONE fp16 plane for every buffer the decoder's convolutions read; `feat` (x_feat, the heads' input) stays split-bf16
        act = plane_f16 if self.precision == "fp16" else planes
        b["x4"] = act(r(h32, w32), 2048, dev, zero=True)
        b["d0"] = torch.empty((N * h32 * w32, 2048), dtype=torch.float32, device=dev)
        cin = 2048
        for (name, _, skip_c, cout), (h, w) in zip(_UP, ((h16, w16), (h8, w8), (h4, w4))):
            b[name + ".in"] = act(r(h, w), round_up(cin + skip_c, 32), dev, zero=True)        # [upsampled | skip | zero pad], zero border
            b[name + ".mid"] = act(r(h, w), cout, dev, zero=True)
            if name != "up3":
                b[name + ".out"] = torch.empty((N * h * w, cout), dtype=torch.float32, device=dev)
            cin = cout
        b["feat"] = planes(r(h4, w4), 256, dev, zero=True)
        return b

    def _features(self, features):
        """The four feature maps the decoder reads, checked: ({index: (N, C, h, w) fp32 contiguous}, N, dims, device)."""
        if self.decoder.training:
            raise lib.MagnetError("DNetMFMA folds BatchNorm running statistics: call .eval() on the D-Net first")
        xs = {}
        for i, c in ((_SKIP_IN, 2048),) + tuple((idx, sc) for _, idx, sc, _ in _UP):
            t = features[i]
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != c:
                raise lib.MagnetError(f"DNetMFMA: features[{i}] must be (N, {c}, h, w), got "
                                      f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if not t.is_cuda:
                raise lib.MagnetError("DNetMFMA: features must be on the GPU (no CPU fallback)")
            xs[i] = t.detach().float().contiguous()
        N = xs[_SKIP_IN].shape[0]
        if any(t.shape[0] != N for t in xs.values()):
            raise lib.MagnetError("DNetMFMA: the feature maps disagree on the batch size")
        dims = tuple(tuple(xs[i].shape[2:]) for i in (_SKIP_IN, 8, 6, 5))
        return xs, N, dims, xs[_SKIP_IN].device

    def _decode(self, xs, N, dims, dev):
        """conv2 and up1..up3 up to the input planes of up3's second convolution (buffers()["up3.mid"]); returns the buffer dict."""
        (h32, w32) = dims[0]
        self.factors_used = []
        self.launch_log = []
        self.packed(dev)
        b = self._buffers(dev, N, dims)

        # conv2 (1x1 2048 -> 2048, no activation; D_dense_depth.py:177) -> compact fp32 for the bilinear upsampling
        f16 = self.precision == "fp16"
        if f16:
            lib.pack_f16(xs[_SKIP_IN], b["x4"], 2048, 0)
        else:
            lib.pack_split(xs[_SKIP_IN], b["x4"][0], b["x4"][1], 2048, 0)
        wp = w32 + 2
        self._conv("conv2", b["x4"], 2048, wp, N * (h32 + 2) * wp, out_f32=b["d0"], border=(h32 + 2, 1), repad=1)
        prev, ph, pw, pc = b["d0"], h32, w32, 2048
        for name, idx, skip_c, cout in _UP:                          # up1..up3 (D_dense_depth.py:178-180)
            h, w = xs[idx].shape[2:]
            wp, rows = w + 2, N * (h + 2) * (w + 2)
            cat = b[name + ".in"]
            cat_ld = cat.shape[1] if f16 else cat[0].shape[1]
            if f16:
                lib.upsample_bilinear_cl_f16(prev, pc, ph, pw, pc, cat, cat_ld, N, h, w, 1)        # channels [0, pc)
                lib.pack_f16(xs[idx], cat, cat_ld, pc)                                             # channels [pc, pc + skip_c)
            else:
                lib.upsample_bilinear_cl(prev, pc, ph, pw, pc, cat[0], cat[1], cat_ld, N, h, w, 1)     # channels [0, pc)
                lib.pack_split(xs[idx], cat[0], cat[1], cat_ld, pc)                                    # channels [pc, pc + skip_c)
            self._conv(name + ".0", cat, cat_ld, wp, rows, dst=b[name + ".mid"], border=(h + 2, 1))
            if name != "up3":
                self._conv(name + ".1", b[name + ".mid"], cout, wp, rows, out_f32=b[name + ".out"], border=(h + 2, 1), repad=1)
                prev, ph, pw, pc = b[name + ".out"], h, w, cout
        return b

    @torch.no_grad()
    def run(self, features, n_ref=None, x_d3_out=None):
        """features: the encoder's list (indices 5, 6, 8, 11 are read; NCHW fp32 on the GPU).
        x_d3_out = (hi, lo, ctot, c_off) with n_ref = B: x_feat of images [0, B) is written into channels [c_off, c_off + 256) of
        the split-bf16 zero-bordered (B*(h+2)*(w+2), ctot) buffer (MAGNET.gnet_input_buffer), border rows zero; returns
        (ref_gmms (B,2,h,w), nghbr_gmms (N-B,2,h,w)).  Without x_d3_out: returns (mono_gmms (N,2,h,w), x_feat (N,256,h,w)) NCHW fp32,
        as the reference's DNET(dnet=False)."""
        xs, N, dims, dev = self._features(features)
        h4, w4 = dims[3]
        if x_d3_out is not None:
            if n_ref is None or not (1 <= int(n_ref) <= N):
                raise lib.MagnetError(f"DNetMFMA: x_d3_out needs n_ref in [1, {N}] (the reference images lead the batch)")
            n_ref = int(n_ref)
            ghi, glo, g_ld, c_off = x_d3_out
            rows_ref = n_ref * (h4 + 2) * (w4 + 2)
            if any(t.dtype != torch.bfloat16 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (rows_ref, g_ld) for t in (ghi, glo)) \
                    or c_off % 8 or c_off < 0 or c_off + 256 > g_ld:
                raise lib.MagnetError(f"DNetMFMA: x_d3_out must be ({rows_ref}, ctot) planes with 256 channels at c_off (multiple of 8)")
        elif n_ref is not None:
            raise lib.MagnetError("DNetMFMA: n_ref goes with x_d3_out (without it run() returns the NCHW (mono_gmms, x_feat))")
        b = self._decode(xs, N, dims, dev)
        # up3's second convolution is x_feat: the reference frames' rows straight into the G-Net buffer, the others into `feat`
        h, w, wp = h4, w4, w4 + 2
        img_rows = (h + 2) * wp
        mid = b["up3.mid"]
        mono = torch.empty((N, 2, h, w), dtype=torch.float32, device=dev)
        parts = []                                                   # (first image, images, planes, row pitch)
        if x_d3_out is not None:
            dst = (ghi[:, c_off:], glo[:, c_off:])
            self._conv("up3.1", mid, 256, wp, n_ref * img_rows, dst=dst, out_ld=g_ld, border=(h + 2, 1))
            parts.append((0, n_ref, dst, g_ld))
        else:
            n_ref = 0
        if N > n_ref:
            src = mid[n_ref * img_rows:] if self.precision == "fp16" else (mid[0][n_ref * img_rows:], mid[1][n_ref * img_rows:])
            dst = (b["feat"][0][n_ref * img_rows:], b["feat"][1][n_ref * img_rows:])
            self._conv("up3.1", src, 256, wp, (N - n_ref) * img_rows, dst=dst, border=(h + 2, 1))
            parts.append((n_ref, N - n_ref, dst, 256))
        # depth head (3x3 + 1x1 + 1x1, one launch) and the Gaussian activation (DNET.py:62-67)
        for first, n, (fhi, flo), ld in parts:
            if any(t.stride(0) != ld or t.shape[0] < n * img_rows or t.shape[1] < 256 for t in (fhi, flo)):
                raise lib.MagnetError(f"DNetMFMA: depth-head input view {tuple(fhi.shape)} does not hold {n * img_rows} x 256 at pitch {ld}")
            work = self._head_work.setdefault(n, {})
            with timed(DNetMFMA.event_sink, 2.0 * n * img_rows * (9 * 256 * 128 + 128 * 128 + 128 * 2)), self._logged("depth_head"):
                out, out_ld = self._head.run(fhi, flo, ld, n * img_rows, wp, work)
            lib.dnet_gauss_head(out, out_ld, n, h, w, 1, mono[first:first + n])
        if x_d3_out is not None:
            return mono[:n_ref], mono[n_ref:]
        x_feat = torch.empty((N, h, w, 256), dtype=torch.float32, device=dev)
        self._conv("up3.1", mid, 256, wp, N * img_rows, out_f32=x_feat, border=(h + 2, 1), repad=1)
        return mono, x_feat.permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def run_standalone(self, features):
        """The stand-alone D-Net behind the encoder: (N, 2, 4h, 4w) fp32 [mu, variance], what the reference's DNET(dnet=True) returns in
        eval mode for these features (D_dense_depth.py:187-192, DNET.py:55-60).  The decoder pass of run(), x_feat kept as split-bf16
        planes, then three launches: the depth head, the mask head (both 3x3 + fused 1x1 tails) and magnet_dnet_upsample_gauss."""
        xs, N, dims, dev = self._features(features)
        if self._mask is None:
            check_decoder(self.decoder, standalone=True)
            mh = self.decoder.mask_head
            # as the depth head: the fused epilogue has two hidden 1x1 layers, the second is the identity behind a ReLU
            self._mask = ConvStackMFMA(nn.Sequential(mh[0], nn.ReLU(), mh[2], nn.ReLU(), self._eye, nn.ReLU(), mh[4]))
            self._mask.small_tiles = False
        b = self._decode(xs, N, dims, dev)
        h, w = dims[3]
        wp = w + 2
        rows = N * (h + 2) * wp
        feat = b["feat"]
        self._conv("up3.1", b["up3.mid"], 256, wp, rows, dst=feat, border=(h + 2, 1))
        sink = DNetMFMA.event_sink
        outs = []
        for stack, work, cout in ((self._head, self._head_work, 2), (self._mask, self._mask_work, 144)):
            with timed(sink, 2.0 * rows * (9 * 256 * 128 + 128 * 128 + 128 * cout)), self._logged("depth_head" if cout == 2 else "mask_head"):
                outs.append(stack.run(feat[0], feat[1], 256, rows, wp, work.setdefault(N, {})))
        (head, head_ld), (mask, mask_ld) = outs
        out = torch.empty((N, 2, 4 * h, 4 * w), dtype=torch.float32, device=dev)
        with timed(sink, 0.0):                                        # not a convolution: bandwidth, no matrix-core work
            lib.dnet_upsample_gauss(head, head_ld, mask, mask_ld, N, h, w, out)
        return out

    def __call__(self, features):
        """(mono_gmms (N,2,h,w), x_feat (N,256,h,w)) NCHW fp32: what the reference's DNET(dnet=False) returns for these features."""
        return self.run(features)
