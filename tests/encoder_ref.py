"""fp64 restatements of the EfficientNet encoder's launches (csrc/enc_kernels.hip and MAGNET_ACT_SILU of csrc/conv_mfma.hip), each with
a pointwise error bound derived from the kernel's arithmetic, and the inputs the GPU tests (tests/test_gpu_encoder.py) share.  The
conventions are those of tests/conv_fwd_ref.py (U, LOLO, gamma_l, check, conv_fwd_ref are imported from there, not copied): every
function takes exactly what the kernel received, returns (ref, bound) as float64 CPU tensors, and no figure is fitted to a measured
error.  u = U = 2^-24, gamma(L) = L u / (1 - L u), LOLO = 2^-16 (the residual of the split hi = bf16(v), lo = bf16(v - hi)).

  sigmoid, SiLU                The kernels compute e = exp2(fl(-x C)), C the fp32 nearest log2(e), on the hardware exponential, then
  (SIG_ABS, SILU_REL,          1 / (1 + e) resp. x / (1 + e): one fp32 addition and one correctly rounded division (build flag).  The
   SILU_ABS)                   instruction errs by E_NATIVE = 1 ulp <= 2 u (tests/elementwise_fwd_ref.py: measured over every input
                               in [-128, 0]); the rounded product and the constant add a relative |x| u D to e, D = C ln2 +
                               |C ln2 - 1| / u = 1.224.  So e is known to d_e = (2 + 1.224 |x|) u relative, and with s = sigmoid(x):
                                   |sigmoid - s| <= s (1 - s) d_e + 2 u s <= (0.5 + 1.224 * 0.2239 + 2) u < 3 u      (|x| s (1 - s) <= 0.2239)
                                   |silu - x s| <= |x s| ((1 - s) 2 u + 2 u) + 1.224 u x^2 s (1 - s) <= 4 u |x s| + 0.55 u   (x^2 s (1 - s) <= 0.44)
                               Where e overflows (x < -88.7) the results are +0 / -0 against |true| < 2^-120; where it is flushed
                               (x > 87.3) they are 1 / x against a relative 2^-126.  include/magnet_hip.h states the rounded-up forms
                               SIG_ABS = 2^-21, SILU_REL = 2^-21, SILU_ABS = 2^-22, and those are what the tests use.  SiLU is
                               1.1-Lipschitz (max |silu'| = 1.0998), the sigmoid 1/4-Lipschitz: an input known to b gives
                                   silu_bound = 1.1 b + SILU_REL (|silu(ref)| + 1.1 b) + SILU_ABS,  sig_bound = b / 4 + SIG_ABS.
  stem (stem_ref)              27 fused multiply-adds and the bias addition, gamma(28) (|w| conv |x| + |b|), then SiLU, then the split:
                               + LOLO (|ref| + bound).  TF "SAME": pad_total = max((ceil(L / 2) - 1) 2 + 3 - L, 0), total // 2 in front.
  depthwise (dwconv_ref)       each input is joined hi + lo in fp32 (one rounding, exact for planes that are a split), k k fused
                               multiply-adds in one accumulator (taps outside the image are skipped), the bias addition:
                               gamma(k k + 2) (|w| conv |x| + |b|); SiLU; the stored planes add LOLO (|ref| + bound).
                               Partial sums: the fp32 outputs v^ (before the split) of one 8 x 16 tile: a thread adds its 4 outputs,
                               the workgroup adds 32 strip sums: every term passes through at most 4 + 32 additions:
                                   |part - sum v| <= sum bound(v) + gamma(36) sum (|v| + bound(v)).
  gate (se_gate_ref)           mean = (sum of n_part partials, in order) * fl(1 / hw): gamma(n_part + 2) sum |part| / hw.
                               reduce: lane l accumulates 4 ceil(C / 256) + 1 fused multiply-adds (channel quads, and the tail of
                               C % 4), 6 butterfly additions, the bias: L1 = 4 ceil(C / 256) + 8 roundings; expand: R fused multiply-adds and the bias: L2 = R + 1.  A layer with
                               inputs a known to e:  |W| e + gamma(L) (|W| (|a| + e) + |b|).  SiLU between them, sigmoid after.
  scale (se_scale_ref)         (hi + lo) in fp32 (one rounding), times the gate (one rounding): gamma(2) |x g|; the split adds LOLO.
  MAGNET_ACT_SILU              conv_fwd_ref's pre-activation and bound, then SiLU as above; out_mode 0 adds the split.
  (conv_silu_ref)
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests.conv_fwd_ref import GUARD, LOLO, U, check, conv_fwd_ref, gamma_l, guarded, join, ratio  # noqa: F401

SIG_ABS = 2.0 ** -21
SILU_REL = 2.0 ** -21
SILU_ABS = 2.0 ** -22
SILU_LIP = 1.1
TILE_H, TILE_W = 8, 16                                 # one depthwise workgroup's output tile = one row of the partial-sum scratch


def same_pad(size, k, stride):
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return total // 2, total - total // 2


def silu_ref(ref, bound):
    s = ref * torch.sigmoid(ref)
    return s, SILU_LIP * bound + SILU_REL * (s.abs() + SILU_LIP * bound) + SILU_ABS


def sigmoid_ref(ref, bound):
    return torch.sigmoid(ref), 0.25 * bound + SIG_ABS


def split_bound(ref, bound):
    return bound + LOLO * (ref.abs() + bound)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def to_grid(x_nchw, c_pad):
    """(N, C, h, w) -> the zero-bordered channel-last grid (N, h+2, w+2, c_pad) in the dtype of x."""
    N, C, h, w = x_nchw.shape
    g = torch.zeros((N, h + 2, w + 2, c_pad), dtype=x_nchw.dtype)
    g[:, 1:h + 1, 1:w + 1, :C] = x_nchw.permute(0, 2, 3, 1)
    return g


def split_planes(g):
    """fp32 grid -> (hi, lo) bf16 planes (rows, c)."""
    flat = g.reshape(-1, g.shape[-1]).float()
    hi = flat.to(torch.bfloat16)
    lo = (flat - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


def interior(planes64, N, h, w):
    """(rows, c) fp64 -> NCHW (N, c, h, w) of the interior."""
    return planes64.reshape(N, h + 2, w + 2, -1)[:, 1:h + 1, 1:w + 1].permute(0, 3, 1, 2)


# ---- the launches ---------------------------------------------------------------------------------------------------------------
def _dw64(x, w, k, stride, pt, pleft):
    """Depthwise correlation in fp64 with explicit top / left padding: x (N, C, h, w), w (C, k, k) -> (N, C, ceil(h/s), ceil(w/s))."""
    N, C, h, wd = x.shape
    ho, wo = -(-h // stride), -(-wd // stride)
    pb, pr = max((ho - 1) * stride + k - h - pt, 0), max((wo - 1) * stride + k - wd - pleft, 0)
    xp = F.pad(x, (pleft, pr, pt, pb))
    return F.conv2d(xp, w[:, None], None, stride, 0, 1, C)[:, :, :ho, :wo]


def dwconv_ref(x, wgt, bias, k, stride, pt, pleft):
    """x (N, c_pad, h, w) fp64 = hi + lo of the input planes' interior; wgt (k*k, c_pad), bias (c_pad) as the kernel received them.
    Returns (ref, bound_fp32, bound_planes): the fp32 value before the split and the stored planes' bound, (N, c_pad, ho, wo)."""
    x, wgt, bias = x.double(), wgt.double(), bias.double()
    w = wgt.t().reshape(-1, k, k)
    pre = _dw64(x, w, k, stride, pt, pleft) + bias[None, :, None, None]
    mag = _dw64(x.abs(), w.abs(), k, stride, pt, pleft) + bias.abs()[None, :, None, None]
    ref, b = silu_ref(pre, gamma_l(k * k + 2) * mag)
    return ref, b, split_bound(ref, b)


def dw_partials_ref(ref, bound):
    """The partial sums (N, n_part, c_pad) of dwconv_ref's fp32 outputs and their bound."""
    N, C, ho, wo = ref.shape
    ty, tx = -(-ho // TILE_H), -(-wo // TILE_W)
    pad = (0, tx * TILE_W - wo, 0, ty * TILE_H - ho)
    def tiles(t):
        t = F.pad(t, pad).reshape(N, C, ty, TILE_H, tx, TILE_W)
        return t.sum((3, 5)).reshape(N, C, ty * tx).permute(0, 2, 1)
    return tiles(ref), tiles(bound) + gamma_l(36) * tiles(ref.abs() + bound)


def se_gate_ref(part, hw, w1, b1, w2t, b2, C, c_pad):
    """part (N, n_part, c_pad) fp32 as the kernel read it.  Returns (gate (N, c_pad), bound)."""
    part, w1, b1, w2t, b2 = (t.double().cpu() for t in (part, w1, b1, w2t, b2))
    N, n_part, _ = part.shape
    R = w1.shape[0]
    m = part[:, :, :C].sum(1) / hw
    e = gamma_l(n_part + 2) * part[:, :, :C].abs().sum(1) / hw
    L1, L2 = 4 * -(-C // 256) + 8, R + 1
    r = m @ w1.t() + b1
    er = e @ w1.abs().t() + gamma_l(L1) * ((m.abs() + e) @ w1.abs().t() + b1.abs())
    r, er = silu_ref(r, er)
    g = r @ w2t + b2
    eg = er @ w2t.abs() + gamma_l(L2) * ((r.abs() + er) @ w2t.abs() + b2.abs())
    g, eg = sigmoid_ref(g, eg)
    gate, bound = torch.zeros((N, c_pad), dtype=torch.float64), torch.zeros((N, c_pad), dtype=torch.float64)
    gate[:, :C], bound[:, :C] = g, eg
    return gate, bound


def se_scale_ref(x, gate):
    """x (N, c_pad, h, w) fp64 = hi + lo of the planes' interior, gate (N, c_pad) fp32 as read.  The stored planes: (ref, bound)."""
    ref = x.double() * gate.double()[:, :, None, None]
    return ref, split_bound(ref, gamma_l(2) * ref.abs())


def stem_ref(img, wgt, bias):
    """img (N, 3, H, W), wgt (48, 27), bias (48) as the kernel received them -> (ref, bound) (N, 48, H2, W2) of the stored planes."""
    img, w, b = img.double().cpu(), wgt.double().cpu().reshape(48, 3, 3, 3), bias.double().cpu()
    (pt, pb), (pl, pr) = same_pad(img.shape[2], 3, 2), same_pad(img.shape[3], 3, 2)
    xp = F.pad(img, (pl, pr, pt, pb))
    pre = F.conv2d(xp, w, b, 2)
    mag = F.conv2d(xp.abs(), w.abs(), b.abs(), 2)
    ref, bd = silu_ref(pre, gamma_l(28) * mag)
    return ref, split_bound(ref, bd)


def conv_silu_ref(x, w, bias, rows, add=None, planes=True):
    """A taps = 1 launch with MAGNET_ACT_SILU: conv_fwd_ref's arguments; planes: the output is split-bf16 (out_mode 0)."""
    pre, b = conv_fwd_ref(x, w, bias, 1, 1, rows, add=add)
    ref, b = silu_ref(pre, b)
    return (ref, split_bound(ref, b)) if planes else (ref, b)


def log2e_constant_term():
    """D of the docstring: the rounded product and the constant's own error, per |x| u."""
    c = float.fromhex("0x1.715476p+0")
    return c * math.log(2.0) + abs(c * math.log(2.0) - 1.0) / U
