"""fp64 restatements of the element-wise FORWARD launches of the default inference step (csrc/elementwise.hip, csrc/fnet_kernels.hip,
csrc/dnet_kernels.hip: dnet_gauss_head), each with a pointwise error bound derived from the kernel's arithmetic, and the inputs the
GPU tests (tests/test_gpu_elementwise_fwd.py) and the CPU tests (tests/test_elementwise_fwd_ref.py) share.  The conventions are those
of tests/conv_fwd_ref.py (U, LOLO, gamma_l, check, check_planes_exact are imported from there, not copied): every function takes
exactly what the kernel received, returns (ref, bound) as float64 CPU tensors, a bound of 0 means bit-exact, and no figure is fitted
to a measured error.  u = U = 2^-24, gamma(L) = L u / (1 - L u), ULP1 = 2 u = a 1-ulp library function (tests/dnet_standalone_ref.py).

  Gaussian update              mu1 = mu0 + o0 * sg0: the product and the sum are one rounding each (no contraction: -ffp-contract=off;
  (gaussian_update_ref)        a fused form would err less): |got - ref| <= u |p| + u (|mu1| + u |p|),  p = o0 sg0.
  both layouts                 sg1 = ((e + 1) + 1e-10f) * sg0 with e = elu(o1) = o1 where o1 > 0 (exact), else expm1f(o1), the 1-ulp library
                               function: ULP1 |e|.  With t = e + 1 + 1e-10: the two additions round values <= t (u t each, to first
                               order), the constant 1e-10f is the fp32 nearest 1e-10 (u 1e-10), the product is one more rounding (u t sg0):
                                   |got - ref| <= (ULP1 |e| [o1 <= 0] + 3 u t + u 1e-10) |sg0| (1 + 4 u).
                               The first term is ABSOLUTE: where e + 1 cancels (o1 far below 0, e -> -1, t -> 1e-10) the bound stays at
                               about 2 u |e| sg0 = 1.2e-7 sg0, a thousand times the 1e-10 sg0 the constant contributes.  An fp64 bound
                               therefore CANNOT see the 1e-10 (a kernel without it passes); the G4 golden comparison of
                               tests/test_gpu_conv.py, whose sigma reaches the floor, keeps that job.
  convex upsampling            out[p, b, c, K y + i, K x + j] = sum_t w[t] depth[p, b, c, y + t // 3 - 1, x + t % 3 - 1] (zero outside),
  (convex_upsample_ref)        w = softmax over the 9 taps of logits[b, t, i, j, y, x]: one restatement for magnet_upsample_depth
  all three entry points       (NCHW logits, channel t K K + i K + j), magnet_upsample_depth_cl and _cl_n (padded channel-last logits,
                               channel t 16 + i 4 + j, K = 4); the entry points differ in addressing only.  The term list is that of
                               dnet_standalone_ref.softmax_tap_terms / convex_sum_bound (shared, not copied): the rounding of x - max,
                               the exponential, the 8 additions of the denominator, the reciprocal, the two products, the 8 additions
                               of the sum of 9, each weighted by w[t] |v[t]|, plus 9 FMIN max|v| for exponentials that underflowed.
                               The exponential here is the NATIVE one: __expf(d) = exp2(fl(C d)) with C = 0x1.715476p+0, the fp32
                               nearest log2(e) (clang's __clang_hip_math.h).  For d^ = d (1 + d1) (the subtraction) and p^ = C d^ (1 + d2)
                               (the product): exp2(p^) / exp(d) = exp(ln2 (p^ - d log2 e)) and
                                   ln2 |p^ - d log2 e| <= |d| (C ln2 (|d1| + |d2|) + |C ln2 - 1|) = |d| u D_ERR,
                                   D_ERR = 2 C ln2 + |C ln2 - 1| / u = 2.224:
                               the subtraction, the product rounding (|d| u each on that tap) and the constant's own error (0.224 |d| u).
                               The instruction's error E_NATIVE (in ulp; 1 ulp <= 2 u relative) is the one number not derived:
                               the vendor's documentation installed with the toolchain does not state it (no mention of an accuracy in ulp
                               under the ROCm install's doc directory), so it was MEASURED with tools/native_exp2_probe.hip: one launch
                               over every fp32 input in [-128, 0] against fp64 exp2 on the host, on an MI355X (gfx950) on 2026-10-20:
                               worst error 0.782712 ulp (at -0.750095963) over the 1123811329 inputs whose result is a normal number ->
                               E_NATIVE = 1, the measured maximum rounded up to the next whole ulp (a property of the instruction, so
                               no further margin); results below 2^-126 are flushed to zero (worst loss 0.999995 * 2^-126: the FMIN
                               term).  E_NATIVE is never calibrated through lib.upsample_depth* itself.
  dnet_gauss_head              channel 0 is copied: bound 0.  Channel 1 = sqrtf(t^) with t^ the fp32 (e + 1) + 1e-10f known to
  (gauss_head_ref)             E_t = ULP1 |e| [o1 <= 0] + 2 u t + u 1e-10 (as above, without the product).  |sqrt a - sqrt b| <= |a - b| / sqrt(b)
                               (for b = t) and <= sqrt |a - b| (always); the correctly rounded square root (build flag) adds u of
                               its result:  bound = s_err + u (sqrt t + s_err),  s_err = min(E_t / sqrt t, sqrt E_t) (1 + 4 u).
  F-Net small layers           The kernels compute in fp32 and store either ONE fp16 rounding (fmt "f16": the `_f16` entry points) or the
  (stem_ref, avgpool_ref,      two-plane split hi = bf16(v), lo = bf16(v - hi) (fmt "planes", the default).  Store term of a value v known
  bilinear_ref), both plane    to `arith`:  f16: 2^-11 |ref| where |ref| >= 2^-14, else 2^-25 (fp16 denormals are kept);  planes: the residual
  formats                      of the split, derived as conv_fwd_ref.py derives LOLO: bf16 keeps 8 bits, so |v - hi| <= 2^-8 |v|; v - hi is
                               exact in fp32 (a multiple of ulp(v) below 2^-8 |v|); its bf16 rounding leaves |v - hi - lo| <= 2^-8 |v - hi|
                               <= 2^-16 |v| = LOLO |v| <= LOLO (|ref| + arith), plus 2^-134 where lo falls into bf16's denormals
                               (kept).  The test reads the planes back as hi + lo in fp64, which adds nothing.
                                 stem       27 fused multiply-adds and the bias addition: gamma(28) (|w| conv |x| + |b|); ReLU is 1-Lipschitz
                                 avgpool    k^2 terms summed in fp32 (16 strided partial sums, then their sum: every term passes through at
                                            most k^2 - 1 additions), then times fl(1 / k^2): gamma(k^2 + 2) mean|x|.  fp16 inputs are exact
                                            in fp32; plane inputs are joined hi + lo in fp32 first, one more rounding: gamma(k^2 + 3)
                                 bilinear   the interpolation weights are formed in fp32 from the integer coordinates exactly as the
                                            kernel forms them (IEEE operations, no contraction: repeated in torch fp32, promoted to fp64),
                                            then ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11): 4 terms, at most 5 roundings on any
                                            path: gamma(6) sum w_i |v_i|
  space_to_depth, pack_gmm     moves: bit for bit (space_to_depth_ref, pack_gmm_ref give the expected image).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.conv_fwd_ref import LOLO, U, check, check_planes_exact, gamma_l, ratio  # noqa: F401
from tests.dnet_standalone_ref import ULP1, convex_sum_bound, softmax_tap_terms

E_NATIVE = 1.0                                       # ulp of v_exp_f32 on gfx950: measured 0.782712 (tools/native_exp2_probe.hip, 2026-10-20), rounded up
LOG2E_F32 = float.fromhex("0x1.715476p+0")           # __expf's constant
D_ERR = 2.0 * LOG2E_F32 * math.log(2.0) + abs(LOG2E_F32 * math.log(2.0) - 1.0) / U      # per |d|, in units of U: 2.224
EPS10 = 1e-10


def _t64(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.detach().cpu().double()


# ---- Gaussian update, dnet_gauss_head ---------------------------------------------------------------------------------------------
def _elu_t(o1):
    """e = elu(o1), t = e + 1 + 1e-10 and the error of the fp32 t before any product: (e, t, E_t)."""
    e = torch.where(o1 > 0, o1, torch.expm1(o1.clamp_max(0.0)))
    t = e + 1.0 + EPS10
    lib_err = torch.where(o1 > 0, torch.zeros_like(e), ULP1 * e.abs())
    return e, t, lib_err + 2.0 * U * t + U * EPS10


def gaussian_update_ref(o, g):
    """o = G-Net output (B, 2, h, w), g = previous [mu, sigma] (B, 2, h, w), both as the kernel read them (either layout's values)."""
    o, g = _t64(o), _t64(g)
    mu0, sg0, o0, o1 = g[:, 0], g[:, 1], o[:, 0], o[:, 1]
    p = o0 * sg0
    mu1 = mu0 + p
    b_mu = U * p.abs() + U * (mu1.abs() + U * p.abs())
    _, t, e_t = _elu_t(o1)
    sg1 = t * sg0
    b_sg = (e_t + U * t) * sg0.abs() * (1.0 + 4.0 * U)
    return torch.stack([mu1, sg1], 1), torch.stack([b_mu, b_sg], 1)


def gauss_head_ref(x):
    """x = the depth head's output (N, 2, h, w) as the kernel read it.  Returns [o0, sqrt(elu(o1) + 1 + 1e-10)] and its bound."""
    x = _t64(x)
    _, t, e_t = _elu_t(x[:, 1])
    s = t.sqrt()
    s_err = torch.minimum(e_t / s, e_t.sqrt()) * (1.0 + 4.0 * U)
    return torch.stack([x[:, 0], s], 1), torch.stack([torch.zeros_like(s), s_err + U * (s + s_err)], 1)


# ---- convex upsampling --------------------------------------------------------------------------------------------------------------
def logits_nchw(mask, K):
    """(B, 9 K K, h, w) -> the (B, 9, K, K, h, w) view."""
    m = np.asarray(mask)
    B, _, h, w = m.shape
    return m.reshape(B, 9, K, K, h, w)


def logits_cl(mask_pad, ld, B, h, w):
    """Padded channel-last rows (B (h+2) (w+2), ld) -> (B, 9, 4, 4, h, w): interior texels, channels [0, 144)."""
    m = np.asarray(mask_pad).reshape(B, h + 2, w + 2, ld)[:, 1:-1, 1:-1, :144]
    return m.reshape(B, h, w, 9, 4, 4).transpose(0, 3, 4, 5, 1, 2)


def convex_upsample_ref(depth, logits):
    """depth (P, B, C, h, w), logits (B, 9, K, K, h, w) -> (ref, bound) (P, B, C, K h, K w)."""
    D = np.asarray(depth, dtype=np.float64)
    L = np.asarray(logits, dtype=np.float64)
    P, B, C, h, w = D.shape
    K = L.shape[2]
    _, wgt, Kt = softmax_tap_terms(L, axis=1, d_err=D_ERR, exp_err=2.0 * E_NATIVE)
    Dp = np.pad(D, ((0, 0), (0, 0), (0, 0), (1, 1), (1, 1)))
    up = np.zeros((P, B, C, K, K, h, w))
    S = np.zeros_like(up)
    vmax = np.zeros((P, B, C, 1, 1, h, w))
    for t in range(9):
        v = Dp[..., t // 3:t // 3 + h, t % 3:t % 3 + w][:, :, :, None, None]
        up += wgt[None, :, None, t] * v
        S += wgt[None, :, None, t] * np.abs(v) * Kt[None, :, None, t]
        vmax = np.maximum(vmax, np.abs(v))
    E = convex_sum_bound(S, Kt, vmax)

    def img(a):
        return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 1, 2, 5, 3, 6, 4)).reshape(P, B, C, h * K, w * K))
    return img(up), img(E)


# ---- the F-Net's small layers -----------------------------------------------------------------------------------------------------------
def _f16_round(ref):
    a = ref.abs()
    return torch.where(a >= 2.0 ** -14, a * 2.0 ** -11, torch.full_like(a, 2.0 ** -25))


def store_term(ref, arith, fmt):
    """The error the store adds to a value known to `arith` (module docstring)."""
    if fmt == "f16":
        return _f16_round(ref)
    if fmt == "planes":
        return LOLO * (ref.abs() + arith) + 2.0 ** -134
    raise ValueError(f"fmt {fmt!r}")


def stem_ref(img, wgt, bias, fmt):
    """img (N, 3, H, W), wgt (32, 27) = [co][ci][dy][dx], bias (32) -> relu(3x3 stride 2, padding 1) as (N, H2, W2, 32)."""
    x, wt, b = _t64(img), _t64(wgt).reshape(32, 3, 3, 3), _t64(bias)
    N, _, H, W = x.shape
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros((N, 3, 2 * H2 + 1, 2 * W2 + 1), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    pre = b.expand(N, H2, W2, 32).clone()
    mag = b.abs().expand(N, H2, W2, 32).clone()
    for dy in range(3):
        for dx in range(3):
            tap = xp[:, :, dy:dy + 2 * H2:2, dx:dx + 2 * W2:2]                        # img[2y + dy - 1, 2x + dx - 1]
            pre += torch.einsum("nchw,oc->nhwo", tap, wt[:, :, dy, dx])
            mag += torch.einsum("nchw,oc->nhwo", tap.abs(), wt[:, :, dy, dx].abs())
    ref = pre.clamp_min(0.0)
    arith = gamma_l(28) * mag
    return ref, arith + store_term(ref, arith, fmt)


def avgpool_ref(x, k, fmt):
    """x (N, h, w, C) = the values of the slice (fp16 values, or hi + lo) -> AvgPool2d(k, k), floor mode, as (N ph pw, C)."""
    x = _t64(x)
    N, h, w, C = x.shape
    ph, pw = h // k, w // k
    win = x[:, :ph * k, :pw * k].reshape(N, ph, k, pw, k, C)
    ref = win.sum(dim=(2, 4)).reshape(-1, C) / (k * k)
    mag = win.abs().sum(dim=(2, 4)).reshape(-1, C) / (k * k)
    arith = gamma_l(k * k + (2 if fmt == "f16" else 3)) * mag
    return ref, arith + store_term(ref, arith, fmt)


def bilinear_axis(n_in, n_out, coords="kernel"):
    """(i0, i1, l0, l1) of every output index.  coords "kernel": the kernel's fp32 coordinate arithmetic, operation by operation;
    "exact": the same rule in float64 (what the kernel-coordinate form is itself checked against on the CPU)."""
    dt = torch.float32 if coords == "kernel" else torch.float64
    s = (torch.tensor(float(n_in - 1), dtype=dt) / torch.tensor(float(n_out - 1), dtype=dt)) if n_out > 1 else torch.tensor(0.0, dtype=dt)
    f = s * torch.arange(n_out, dtype=dt)
    i0 = f.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = f - i0.to(dt)
    return i0, i1, (1.0 - l1).double(), l1.double()


def bilinear_ref(q, h, w, fmt, coords="kernel"):
    """q (N, ph, pw, C) fp32 values -> bilinear, align_corners=True, (N, h, w, C)."""
    qd = _t64(q)
    y0, y1, ly0, ly1 = bilinear_axis(qd.shape[1], h, coords)
    x0, x1, lx0, lx1 = bilinear_axis(qd.shape[2], w, coords)
    terms = [(ly0[:, None] * lx0[None, :], qd[:, y0][:, :, x0]), (ly0[:, None] * lx1[None, :], qd[:, y0][:, :, x1]),
             (ly1[:, None] * lx0[None, :], qd[:, y1][:, :, x0]), (ly1[:, None] * lx1[None, :], qd[:, y1][:, :, x1])]
    ref = sum(wt[None, :, :, None] * v for wt, v in terms)
    mag = sum(wt[None, :, :, None] * v.abs() for wt, v in terms)
    arith = gamma_l(6) * mag
    return ref, arith + store_term(ref, arith, fmt)


def space_to_depth_ref(x):
    """x (N, H2, W2, C) of any dtype -> (N, H4, W4, 4 C): channel (py 2 + px) C + c = x[2y + py, 2x + px, c], zero beyond the edge."""
    N, H2, W2, C = x.shape
    H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
    xs = torch.zeros((N, 2 * H4, 2 * W4, C), dtype=x.dtype)
    xs[:, :H2, :W2] = x
    return torch.cat([xs[:, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=3)


def pack_gmm_ref(g):
    """g (N, 2, h, w) -> (N, h + 2, w + 2, 2) interleaved, zero border."""
    N, _, h, w = g.shape
    out = torch.zeros((N, h + 2, w + 2, 2), dtype=g.dtype)
    out[:, 1:-1, 1:-1] = g.permute(0, 2, 3, 1)
    return out


# ---- the cases and inputs that the GPU tests and the CPU tests share -------------------------------------------------------------------
UPSAMPLE_KC = [(K, C) for K in (1, 2, 4, 8) for C in (1, 2)]
UPSAMPLE_SHAPES = [(1, 1, 1), (2, 6, 67), (3, 9, 37)]                  # w = 67 crosses the 64-lane block, h = 6, 9 the 4-row block
UPSAMPLE_CL_CASES = [(1, 1, 1, 144, 1), (2, 5, 7, 160, 3), (3, 9, 37, 148, 2), (1, 3, 5, 144, 64)]      # B, h, w, ld, n_pred
GAUSS_SHAPES = [(1, 1, 1), (3, 7, 37), (2, 16, 16)]
GAUSS_LDS = [2, 16]
GAUSS_HEAD_CASES = [(1, 1, 1, 0, 2), (3, 7, 11, 1, 16), (2, 5, 9, 2, 6)]                               # N, h, w, pad, in_ld
STEM_SHAPES = [(1, 2, 2), (2, 37, 50), (1, 8, 6)]
S2D_CASES = [(H2, W2, opad) for (H2, W2) in ((11, 14), (1, 1), (8, 9)) for opad in (1, 2)]
AVGPOOL_CASES = [(C, k) for C in (8, 64, 128) for k in (8, 16)]
AVGPOOL_GRID = (2, 19, 35, 2, 320, 64)                                  # N, h, w, pad, ld, channel offset of the slice
BILINEAR_CASES = [(ph, pw, h, w, pad) for (ph, pw, h, w) in ((1, 1, 5, 7), (1, 2, 1, 9), (3, 5, 12, 16), (2, 2, 2, 2)) for pad in (1, 2)]
BILINEAR_N, BILINEAR_C, BILINEAR_LD, BILINEAR_OFF = 2, 32, 320, 224
PACK_GMM_SHAPES = [(1, 1, 1), (3, 13, 21)]
MASK_FILL = 3.0e4                                                       # border rows / spare channels of a padded mask: would win every softmax
O1_SPECIAL = [-20.0, 0.0, 1e-30, -1e-30, 30.0, -90.0, 1e-6, -1e-6, -25.0, -200.0, -0.0, 17.5]


def upsample_inputs(B, h, w, K, C, P=1):
    """(depth (P, B, C, h, w), logits (B, 9 K K, h, w)) fp32: logits N(0, 3^2) with +-80 planted at 2 % each, depth heavy-tailed, both signs."""
    rng = np.random.default_rng([41, B, h, w, K, C, P])
    depth = (rng.standard_normal((P, B, C, h, w)) ** 3 * 2.0).astype(np.float32)
    logits = (rng.standard_normal((B, 9 * K * K, h, w)) * 3.0).astype(np.float32)
    sel = rng.random(logits.shape)
    sel.reshape(B, 9, K * K, h, w)[0, :, 0, 0, 0] = 0.5                 # sub-pixel (0, 0) of the first pixel keeps an ordinary softmax: the
    logits[sel < 0.02] = 80.0                                           # 1 x 1 case at K = 1 has no other, and a planted tap hides its weights
    logits[sel > 0.98] = -80.0
    return depth, logits


def pad_cl(x_nchw, ld, pad=1, fill=0.0):
    """(N, C, h, w) -> padded channel-last rows (N (h+2 pad) (w+2 pad), ld), channels [0, C) of the interior; everything else `fill`."""
    x = np.asarray(x_nchw)
    N, C, h, w = x.shape
    out = np.full((N, h + 2 * pad, w + 2 * pad, ld), fill, dtype=x.dtype)
    out[:, pad:pad + h, pad:pad + w, :C] = x.transpose(0, 2, 3, 1)
    return out.reshape(-1, ld)


def upsample_cl_inputs(B, h, w, ld, n_pred):
    """(depths (n_pred, B, 2, h, w), mask_pad rows (.., ld), logits (B, 144, h, w)): the inputs of upsample_inputs(K=4, C=2, P=n_pred)
    with the mask in the padded channel-last layout, its border rows and spare channels holding MASK_FILL (never read)."""
    depth, logits = upsample_inputs(B, h, w, 4, 2, P=n_pred)
    return depth, pad_cl(logits, ld, fill=np.float32(MASK_FILL)), logits


def gaussian_inputs(B, h, w):
    """(o, g) (B, 2, h, w) fp32: o1 across the ELU knee (O1_SPECIAL planted at every 5th element, N(0, 3^2) elsewhere), sg0 log-uniform
    over 1e-4 .. 1e2, o0 heavy-tailed, mu0 N(0, 3^2)."""
    rng = np.random.default_rng([42, B, h, w])
    n = B * h * w
    o1 = (rng.standard_normal(n) * 3.0).astype(np.float32)
    idx = np.arange(0, n, 5)
    o1[idx] = np.asarray(O1_SPECIAL, dtype=np.float32)[(idx // 5) % len(O1_SPECIAL)]
    o0 = (rng.standard_normal(n) ** 3).astype(np.float32)
    mu0 = (rng.standard_normal(n) * 3.0).astype(np.float32)
    sg0 = (10.0 ** rng.uniform(-4.0, 2.0, n)).astype(np.float32)
    o = np.stack([o0.reshape(B, h, w), o1.reshape(B, h, w)], 1)
    g = np.stack([mu0.reshape(B, h, w), sg0.reshape(B, h, w)], 1)
    return o, g


def gauss_head_inputs(N, h, w):
    """The depth head's (N, 2, h, w) fp32 output: channel 0 heavy-tailed, channel 1 the o1 of gaussian_inputs."""
    o, _ = gaussian_inputs(N, h, w)
    return o


def stem_inputs(N, H, W):
    g = torch.Generator().manual_seed(1000 + 100 * N + H)
    return torch.randn(N, 3, H, W, generator=g), torch.randn(32, 27, generator=g) * 0.2, torch.randn(32, generator=g)


def s2d_inputs(H2, W2, N=2, C=32):
    """Two independent (N, H2, W2, C) fp32 tensors (hi and lo planes of the default format are moved independently)."""
    g = torch.Generator().manual_seed(2000 + 10 * H2 + W2)
    return torch.randn(N, H2, W2, C, generator=g) * 3, torch.randn(N, H2, W2, C, generator=g) * 0.01


def avgpool_inputs():
    """The whole (N, h + 2 pad, w + 2 pad, ld) fp32 buffer: every channel and the border hold data."""
    N, h, w, pad, ld, _ = AVGPOOL_GRID
    return torch.randn(N, h + 2 * pad, w + 2 * pad, ld, generator=torch.Generator().manual_seed(3000)) * 4


def bilinear_inputs(ph, pw):
    """The input rows (N ph pw + pw + 1, C) fp32: the rows behind the last image are NaN (a y1 or x1 past the grid would read them)."""
    q = torch.full((BILINEAR_N * ph * pw + pw + 1, BILINEAR_C), float("nan"))
    q[:BILINEAR_N * ph * pw] = torch.randn(BILINEAR_N * ph * pw, BILINEAR_C, generator=torch.Generator().manual_seed(4000 + 10 * ph + pw))
    return q


def pack_gmm_inputs(N, h, w):
    return torch.randn(N, 2, h, w, generator=torch.Generator().manual_seed(5000 + N))
