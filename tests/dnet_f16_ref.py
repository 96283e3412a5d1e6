"""A torch float64 restatement of the DenseDepth_BN decoder as DNetMFMA(precision="fp16") stores it: every convolution and the
bilinear upsampling are float64 arithmetic, and a value is rounded exactly where the mode rounds it —
    to fp16 (saturating, magnet_amd.planes.to_f16_sat):  the encoder features, the BatchNorm-folded weights, the upsampled slices,
                                                         every up*.0 output;
    to fp32:                                              the biases, conv2's output and up1 / up2's outputs (the compact hand-overs);
    through the bf16 split (hi + lo of the fp32 value):   x_feat.
The heads run in float64 on that x_feat.  Its distance from the plain float64 decoder is what the FORMAT costs; the HIP mode differs
from this restatement only by fp32 accumulation order and by the ties that flip under it."""
import copy

import torch
import torch.nn.functional as F

from magnet_amd.dnet import _SKIP_IN, _UP, gaussian_activation
from magnet_amd.planes import fold_bn, split_bf16, to_f16_sat


def r16(x):
    """Round to fp16 as the mode does (through fp32, saturating), returned as float64."""
    return to_f16_sat(x.float()).double()


def r32(x):
    return x.float().double()


def decoder_f16_ref(decoder, feats):
    """(gmm (N,2,h,w) [mu, sigma], x_feat (N,256,h,w)) in float64.  decoder: an eval-mode DenseDepthDecoder (any dtype; its tensors
    are read as float64); feats: the encoder's fp32 feature list."""
    slope = float(torch.tensor(decoder.up1._net[2].negative_slope, dtype=torch.float32))
    x = F.conv2d(r16(feats[_SKIP_IN].float()), r16(decoder.conv2.weight.detach().double()), r32(decoder.conv2.bias.detach().double()))
    x = r32(x)                                                               # d0: compact fp32
    for name, idx, _, _ in _UP:
        net = getattr(decoder, name)._net
        skip = feats[idx].float()
        up = F.interpolate(x, size=list(skip.shape[2:]), mode="bilinear", align_corners=True)
        cat = torch.cat([r16(up), r16(skip)], dim=1)
        w, b = fold_bn(net[0], net[1])
        mid = r16(F.leaky_relu(F.conv2d(cat, r16(w), r32(b), padding=1), slope))
        w, b = fold_bn(net[3], net[4])
        x = r32(F.leaky_relu(F.conv2d(mid, r16(w), r32(b), padding=1), slope))
    hi, lo = split_bf16(x.float())
    x_feat = hi.double() + lo.double()
    gmm, _ = gaussian_activation((copy.deepcopy(decoder.depth_head).double()(x_feat), None))
    return gmm, x_feat
