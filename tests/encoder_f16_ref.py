"""The fp16 single-plane forms of the EfficientNet encoder's launches (magnet_enc_stem_f16, magnet_dwconv_cl_f16, magnet_se_scale_f16,
magnet_conv_mfma_f16e): the fp64 restatements and bounds of tests/encoder_ref.py (imported, not copied), with the storage format's own
terms in place of the split's, and the CPU emulation of the whole mode.  No figure is fitted to a measured error.

  store (f16_store)            an fp32 result known to `bound` leaves as ONE fp16 value, round to nearest even, 11 significant bits:
                               + 2^-11 |ref|; below 2^-14 fp16 is subnormal with spacing 2^-24: + 2^-25 there (the form of
                               tests/test_gpu_conv_f16p.py).  The test inputs stay far inside |x| <= 65504: no clamp takes part.
  inputs                       every plane the tests pass is exactly fp16-representable and is read exactly (fp16 -> fp32): no input error.
  stem (stem_ref)              encoder_ref's arithmetic (27 fused multiply-adds and the bias, gamma(28); SiLU), then the store.
  depthwise (dwconv_ref)       encoder_ref.dwconv_ref's fp32 value and bound (gamma(k k + 2): the (hi, lo) form's join rounding does
                               not exist here, the bound is kept as it is), then the store.  The partial sums are taken from the fp32
                               values before the store: encoder_ref.dw_partials_ref unchanged — today's bound.
  scale (se_scale_ref)         x * gate: x exact, one rounding: gamma(2) |x g| as today (kept), then the store.
  1x1 layers (conv_ref)        the fp64 convolution of exactly the fp16 planes passed in: every product is exact in the fp32
                               accumulator, so what is left is K = cin accumulator roundings and the epilogue's additions (residual,
                               bias) inside L = K + 4: gamma(K + 4) (|x| conv |w| + |res| + |bias|), the form of
                               tests/test_gpu_conv_f16p.py; then SiLU (2^-21 |silu| + 2^-22 on top of the 1.1-Lipschitz propagation,
                               encoder_ref.silu_ref), then the store for out_mode 3.

  the whole mode (emulate)     an fp64 forward of the torch module with forward hooks that round to fp16 at the five storage points
                               (stem output, expanded tensor, depthwise output, scaled tensor, block output = the residual stream) and
                               with the 1x1 weights rounded to fp16 after the BatchNorm fold (w' = f16(w s) / s in the unfolded module,
                               exact to fp64).  Independent of the code under test: it uses the torch modules only.
"""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F

from tests import encoder_ref as R
from tests.conv_fwd_ref import LOLO, conv_ref, gamma_l

F16_EPS = 2.0 ** -11
F16_TINY = 2.0 ** -14
F16_SUB = 2.0 ** -25


def f16_store(ref, bound):
    a = ref.abs()
    return bound + torch.where(a >= F16_TINY, a * F16_EPS, torch.full_like(a, F16_SUB))


def f16_exact(x):
    """x rounded to fp16 and back: the tests' inputs are exactly representable."""
    return x.to(torch.float16).float()


def to_plane(x_nchw, c_pad):
    """(N, C, h, w) of fp16-representable values -> ONE zero-bordered fp16 plane (rows, c_pad) and its fp64 image."""
    g = R.to_grid(x_nchw, c_pad).reshape(-1, c_pad).to(torch.float16).contiguous()
    return g, g.double()


def stem_ref(img, wgt, bias):
    img, w, b = img.double().cpu(), wgt.double().cpu().reshape(48, 3, 3, 3), bias.double().cpu()
    (pt, pb), (pl, pr) = R.same_pad(img.shape[2], 3, 2), R.same_pad(img.shape[3], 3, 2)
    xp = F.pad(img, (pl, pr, pt, pb))
    pre = F.conv2d(xp, w, b, 2)
    mag = F.conv2d(xp.abs(), w.abs(), b.abs(), 2)
    ref, bd = R.silu_ref(pre, gamma_l(28) * mag)
    return ref, f16_store(ref, bd)


def dwconv_ref(x, wgt, bias, k, stride, pt, pleft):
    """(ref, bound_fp32, bound_plane): encoder_ref.dwconv_ref with the fp16 store in place of the split."""
    ref, b32, _ = R.dwconv_ref(x, wgt, bias, k, stride, pt, pleft)
    return ref, b32, f16_store(ref, b32)


def se_scale_ref(x, gate):
    ref = x.double() * gate.double()[:, :, None, None]
    return ref, f16_store(ref, gamma_l(2) * ref.abs())


def conv_ref_f16(x16, w16, bias, wp, rows, res=None, silu=False, plane=True):
    """A taps = 1 launch of magnet_conv_mfma_f16e: x16 (R, >= cin), w16 (1, cout, cin), res (>= rows, >= cout) the fp64 images of the fp16
    planes, bias (cout) fp32.  (ref, bound) (rows, cout) of the fp32 result (plane=False) or of the stored fp16 plane."""
    cout, K = w16.shape[1], w16.shape[2]
    conv, b0 = conv_ref(x16, w16, 1, wp, rows)
    mag = b0 / (1.01 * LOLO + 1.02 * gamma_l(3 * K + 2))              # conv_ref's |x| conv |w|
    bias = bias.double()[:cout]
    ref, terms = conv, bias.abs().expand_as(conv).clone()
    if res is not None:
        r = res[:rows, :cout].double()
        ref, terms = ref + r, terms + r.abs()
    ref = ref + bias
    bound = gamma_l(K + 4) * (mag + terms)
    if silu:
        ref, bound = R.silu_ref(ref, bound)
    return (ref, f16_store(ref, bound)) if plane else (ref, bound)


# ---- the whole mode ------------------------------------------------------------------------------------------------------------------
def _r16(t):
    return t.to(torch.float16).to(t.dtype)


def emulate(encoder, img):
    """The feature list of an fp64 forward of `encoder` (a torch-backend magnet_amd.encoder.Encoder, eval mode; it is copied, not
    changed) under the fp16 mode's storage: see the module docstring."""
    from magnet_amd.encoder import blocks_of
    enc = copy.deepcopy(encoder).double().eval()
    m = enc.original_model
    rnd = lambda _mod, _inp, out: _r16(out)

    def round_weight(conv, bn):
        with torch.no_grad():
            if bn is None:
                conv.weight.copy_(_r16(conv.weight))
                return
            s = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).view(-1, 1, 1, 1)
            conv.weight.copy_(_r16(conv.weight * s) / s)

    m.act1.register_forward_hook(rnd)                                  # the stem's output
    for _name, blk, ds in blocks_of(m):
        if ds:
            blk.act1.register_forward_hook(rnd)                        # depthwise output
            round_weight(blk.conv_pw, blk.bn2)
        else:
            blk.act1.register_forward_hook(rnd)                        # expanded tensor
            blk.act2.register_forward_hook(rnd)                        # depthwise output
            round_weight(blk.conv_pw, blk.bn1)
            round_weight(blk.conv_pwl, blk.bn3)
        blk.se.register_forward_hook(rnd)                              # scaled tensor
        blk.register_forward_hook(rnd)                                 # block output: the residual stream
    round_weight(m.conv_head, None)
    with torch.no_grad():
        return enc(img.double())
