"""fp64 restatements of conv_mfma's FORWARD launches (csrc/conv_mfma.hip: the plain epilogue, the border / repad addressing, and the fused
1x1 tail), each with a pointwise error bound derived from the kernel's arithmetic.  The checker, the tap
offsets and the fp64 contraction are those of tests/fnet_bwd_ref.py (imported, not copied); the notation is the same: u = 2^-24,
gamma_L = L u / (1 - L u), 2^-16 = LOLO, a bound of 0 means bit-exact.

Every function takes exactly what the kernel received (split planes joined as hi + lo in fp64, so the split of an INPUT is never
counted as error), works on the device of its inputs in float64 and uses matrix products only.

  plain epilogue               got = act(((acc + ad) + bias)) with acc the K loop's fp32 accumulator, K = taps * cin, ad the addend or
  (conv_fwd_ref)               the residual hi + lo (0 when there is neither), act = identity, ReLU or LeakyReLU.
                               acc: each product x w runs as lo hi + hi lo + hi hi on the matrix cores (bf16 products are exact in
                               fp32); the dropped lo lo is <= 2^-8 |x| 2^-8 |w| = LOLO |x w|, and 1.01 covers |hi| <= (1 + 2^-8) |x|.
                               The three partial products of K terms meet in one fp32 accumulator: conv_ref's chain of 3 K + 2
                               roundings, then the two additions of the epilogue: L = 3 K + 4 roundings of a sum whose terms are the
                               3 K partial products (<= 1.02 |x| conv |w| in all), |ad| and |bias|.  The fp32 store is exact.  So
                                   |pre - ref| <= 1.01 LOLO M + 1.02 gamma_L (M + |ad| + |bias|),   M = |x| conv |w|.
                               (LOLO multiplies M alone: nothing is dropped from ad or bias.  A launch with a fused tail starts the
                               accumulator at the addend and adds the bias after it: 3 K + 1 roundings, inside the same L.)
                               Residual: ad = hi + lo formed in fp32.  For planes that are the split of an fp32 value v (every producer
                               in this project: hi = bf16(v), lo = bf16(v - hi)) the sum is EXACT: v - hi is a multiple of ulp(v)
                               below 2^-8 |v|, its bf16 rounding still is, so hi + lo is a multiple of ulp(v) below 2 |v|'s binade
                               end: 24 bits.  For arbitrary planes (lo far below hi) it is one rounding; the bound charges that one
                               rounding, u |hi + lo|, always, so the reference holds for any planes the API accepts.
                               ReLU is 1-Lipschitz and exact in fp32: the bound carries through unchanged.
                               LeakyReLU(s) (s the fp32 the kernel receives; any finite s, negative or above 1, is accepted) is
                               max(1, |s|)-Lipschitz, and the kernel's x * s where x < 0 is one rounding of a value of magnitude
                               <= |s| (|pre| + bound): bound' = max(1, |s|) bound + u |s| (|pre| + bound) wherever pre - bound < 0.
  border, repad                border=(hp, pad): outputs at the border positions of the (N, hp, wp) grids are written as +0 exactly.
  (border_and_repad)           repad = q + 1: only interior positions are written, at row (n (h + 2q) + y + q) (w + 2q) + x + q of
                               an (N, h + 2q, w + 2q) grid; every other element of the output buffer is never touched.
  fused tail                   three 1x1 layers over K = 128 on an LDS-resident activation that is re-split to hi + lo between
  (tail_ref)                   layers.  For an input activation a known to e pointwise: ref' = W a + b and
                                   bound' = |W| e + c_K (|W| (|a| + e) + |b|),   c_K = 1.01 LOLO + 1.02 gamma(3 * 128 + 4):
                               the first term is the propagated input error (interval arithmetic), the second the layer's own
                               arithmetic on the operands it actually holds (magnitude <= |a| + e): 3 * 128 accumulator roundings
                               and the bias addition, inside the plain form's L.  A hidden layer applies ReLU (1-Lipschitz) and
                               re-splits its output v to hi + lo: |v - (hi + lo)| <= LOLO |v| <= LOLO (|relu(ref')| + bound').
                               The tail's input is the first layer's fp32 result split the same way: bound0 = bound + LOLO (|a0| +
                               bound); for an input that IS planes (a0 = hi + lo): bound0 = 0.
"""
from __future__ import annotations

import torch

from tests.fnet_bwd_ref import LOLO, U, check, check_planes_exact, conv_ref, gamma_l, join, ratio, tap_offsets  # noqa: F401

GUARD = 4096                                      # sentinel elements in front of and behind every output buffer of the GPU tests


def guarded(shape, gpu, dtype=torch.float32, fill=float("nan")):
    """A sentinel-filled tensor with GUARD sentinel elements on either side of it (same allocation)."""
    n = 1
    for d in shape:
        n *= int(d)
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=gpu)
    return buf, buf[GUARD:GUARD + n].view(shape)

TAIL_K = 128


def f32(v: float) -> float:
    """The fp32 value a C float argument receives."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def conv_fwd_ref(x, w, bias, taps, wp, rows, dil=1, addend=None, add=None, relu=False, leaky=None):
    """The plain epilogue in fp64.  x (R, >= cin) the rows from the kernel's input pointer (hi + lo), w (taps, cout, cin) (hi + lo of the
    pack), bias (cout); addend (>= rows, >= cout) fp32 or add (>= rows, >= cout) = hi + lo of the residual planes (not both: the API
    rejects the pair); leaky = slope.  Returns (ref, bound) (rows, cout); rows of x outside [0, R) read as zero."""
    if addend is not None and add is not None:
        raise ValueError("addend and the residual exclude each other (MAGNET_E_DIM)")
    cout, cin = w.shape[1], w.shape[2]
    K = taps * cin
    ref, b0 = conv_ref(x, w, taps, wp, rows, dil)
    mag = b0 / (1.01 * LOLO + 1.02 * gamma_l(3 * K + 2))             # conv_ref's |x| conv |w|
    bias = bias.double()[:cout]
    extra = torch.zeros_like(ref)
    terms = bias.abs().expand_as(ref).clone()
    ad = addend if addend is not None else add
    if ad is not None:
        a = ad[:rows, :cout].double()
        ref = ref + a
        terms += a.abs()
        if add is not None:
            extra = U * a.abs()
    ref = ref + bias
    bound = 1.01 * LOLO * mag + 1.02 * gamma_l(3 * K + 4) * (mag + terms) + extra
    if relu:
        ref = ref.clamp_min(0.0)
    elif leaky is not None:
        s = f32(leaky)
        neg = ref - bound < 0
        bound = max(1.0, abs(s)) * bound + torch.where(neg, U * abs(s) * (ref.abs() + bound), torch.zeros_like(bound))
        ref = torch.where(ref < 0, ref * s, ref)
    return ref, bound


def interior(N, hp, wp, pad, device=None):
    m = torch.zeros((N, hp, wp), dtype=torch.bool, device=device)
    m[:, pad:hp - pad, pad:wp - pad] = True
    return m.reshape(-1)


def border_and_repad(ref, bound, N, hp, wp, pad, repad=0):
    """The expected image of the output buffer of a launch with border=(hp, pad) (and repad): (ref, bound, written), each over the rows
    of the OUTPUT buffer.  repad = 0: the N*hp*wp input rows, border positions exactly zero (bound 0), all written.  repad = q + 1: the
    rows of the (N, h + 2q, w + 2q) grid, the interior rows re-addressed; written is False on that grid's border, which keeps whatever
    the buffer held."""
    inner = interior(N, hp, wp, pad, ref.device)
    C = ref.shape[1]
    if not repad:
        z = torch.zeros_like(ref[:N * hp * wp])
        keep = inner[:, None]
        return torch.where(keep, ref[:N * hp * wp], z), torch.where(keep, bound[:N * hp * wp], z), torch.ones_like(inner)
    q, h, w = repad - 1, hp - 2 * pad, wp - 2 * pad
    oref = torch.zeros((N, h + 2 * q, w + 2 * q, C), dtype=torch.float64, device=ref.device)
    obound = torch.zeros_like(oref)
    written = torch.zeros((N, h + 2 * q, w + 2 * q), dtype=torch.bool, device=ref.device)
    oref[:, q:q + h, q:q + w] = ref[:N * hp * wp][inner].reshape(N, h, w, C)
    obound[:, q:q + h, q:q + w] = bound[:N * hp * wp][inner].reshape(N, h, w, C)
    written[:, q:q + h, q:q + w] = True
    return oref.reshape(-1, C), obound.reshape(-1, C), written.reshape(-1)


def c_tail() -> float:
    return 1.01 * LOLO + 1.02 * gamma_l(3 * TAIL_K + 4)


def split_bound(a, bound):
    """Error of an fp32 value known to `bound` after its re-split to hi + lo planes."""
    return bound + LOLO * (a.abs() + bound)


def tail_ref(a0, bound0, tail_w, tail_bias, tail_cout):
    """relu(1x1 128->128), relu(1x1 128->128), 1x1 128->tail_cout on the activation a0 (rows, 128) known to bound0 pointwise.  tail_w:
    hi + lo of the three layers' [cout][128] weights concatenated (flat), tail_bias: 128 + 128 + tail_cout.  Returns (ref, bound) (rows,
    tail_cout): every padded output channel is part of the contract."""
    a, e = a0.double(), bound0.double()
    tail_w, tail_bias = tail_w.double().reshape(-1), tail_bias.double().reshape(-1)
    c = c_tail()
    wo = bo = 0
    for layer, n in enumerate((TAIL_K, TAIL_K, tail_cout)):
        W = tail_w[wo:wo + n * TAIL_K].reshape(n, TAIL_K)
        b = tail_bias[bo:bo + n]
        wo, bo = wo + n * TAIL_K, bo + n
        ref = a @ W.T + b
        bound = e @ W.abs().T + c * ((a.abs() + e) @ W.abs().T + b.abs())
        if layer == 2:
            return ref, bound
        a = ref.clamp_min(0.0)
        e = split_bound(a, bound)
