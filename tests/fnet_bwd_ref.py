"""fp64 restatements of the F-Net backward's launches (magnet_amd/train_fnet.py, csrc/train_fnet_bwd.hip, the weight gradient of
csrc/train_bwd.hip and conv_mfma as the backward calls it), each with a pointwise error bound derived from the kernel's arithmetic,
and a checker that asserts |got - ref| <= bound everywhere and returns the worst ratio |got - ref| / bound.

Every function takes exactly what the kernel received (split planes are rebuilt as hi + lo in fp64, so the split of an input is not
counted as error) and works on the device of its inputs in float64 (matrix products only: no float64 convolution reaches MIOpen).
Notation: u = 2^-24 (fp32 unit roundoff), a chain of L roundings costs at most gamma_L = L u / (1 - L u) of the sum of |terms|
(Higham, Accuracy and Stability of Numerical Algorithms, 3.1).  A bound of 0 means bit-exact.

  conv (conv_mfma, bf16x3)     |got - ref| <= (1.01 * 2^-16 + 1.02 gamma_L) (|a| conv |b| + |addend|), L = 3 K + 2.
                               Each product a b runs as hi hi + hi lo + lo hi on the matrix cores (bf16 products are exact in
                               fp32); the dropped lo lo is <= 2^-8 |a| 2^-8 |b| (bf16 keeps 8 significant bits: |a - hi| <= 2^-8 |a|;
                               the typical 2^-18 is not a bound, and a sum of four terms meets 2^-17); the three partial products
                               of K = taps * cin terms meet in one fp32 accumulator that starts at the addend: 3 K + 1 additions
                               on any path, one more for the store.  (1.01, 1.02: |hi|, |lo| <= (1 + 2^-8) |hi + lo|.)
  wgrad (magnet_wgrad_ex)      the same with L = 3 min(P, 2048) + ceil(P / 2048) + 1: per 2048-row chunk one fp32 accumulator
                               (3 MFMA products per row), then the chunks' fp32 partials summed in order.
  bn_train_backward            dbeta = sum g', dgamma = sum g' xhat with xhat the kernel's own fp32 (x - mean) invstd: fp64 sums
                               of n terms (n 2^-52 of sum |.|) and one fp32 store (u).  dx = gamma invstd (g' - mean g' - xhat mean
                               g' xhat): fp64 arithmetic, one fp32 rounding (u) and the hi + lo split of the output (<= 2^-16), so
                               |gamma invstd| ((2^-16 + 2u)(|g'| + |mean g'| + |xhat mean g' xhat|) + n 2^-52 (mean |g'| + |xhat|
                               mean |g' xhat|)).  ReLU mask: g' = g where t = xhat gamma + beta > 0, t as the kernel rounds it in
                               fp32 (|t_fp32 - t| <= 2u (|xhat gamma| + |beta|)).  Where |t| <= 4u (|xhat gamma| + |beta|) the
                               position is marginal: its own dx may follow either mask, and every bound of its channel widens by
                               what its flip moves the two means.  Passing the forward's mask instead (mask=) makes it exact.
  spp_upsample_backward        the fp64 gradient of F.interpolate(bilinear, align_corners=True); the kernel sums each pooled
                               cell's window in fp32 along a chain of L = Lx + Ly / 8 + 12 roundings (row sums of <= Lx terms, one
                               product per row, eight row slices of <= Ly / 8 rows, then the eight slices), with fp32 1-D weights
                               whose absolute error is <= eps = 4u (in_n + 1) (f = s o rounded twice, then f - floor f): bound
                               1.01 gamma_L sum |w g| + (eps_y + eps_x + eps_y eps_x) sum over the two-cell support of |g|.
  spp_pool_backward            out = g + sum over the branches of dpool / k^2 where floor pooling covers the position: k^2 is a
                               power of two (exact), four fp32 additions: 8u (|g| + sum |dpool / k^2|) where a branch covers, and
                               bit-exact (bound 0) in the remainder band that no branch covers.
  fnet_stem_wgrad              each stage-1 workgroup sums its <= ceil(P / 256) positions in fp32 (one product and one addition
                               each: L = ceil(P / 256) + 1), the dz operand is hi + lo rounded to fp32 (u); the 256 partials meet in
                               fp64, one fp32 store: ((L + 1) u + u) * 1.01 * sum |dz img|.
  fnet_grad_pack, d2s_backward bit-exact: split_bf16 of the input (NaN stays NaN), and a gather.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
LOLO = 2.0 ** -16                    # |lo| <= 2^-8 |v|: the dropped lo lo product, and the residual of a hi + lo split


def gamma_l(L: int) -> float:
    return L * U / (1.0 - L * U)


def join(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    """Split planes -> fp64 hi + lo."""
    return hi.double() + lo.double()


def tap_offsets(taps: int, wp: int, dil: int = 1):
    """Row offsets of the grid taps: 3x3 (dilated), the space-to-depth 2x2 window, or 1x1."""
    d = max(int(dil), 1)
    if taps == 9:
        return [((t // 3 - 1) * wp + (t % 3 - 1)) * d for t in range(9)]
    if taps == 4:
        return [-wp - 1, -wp, -1, 0]
    if taps == 1:
        return [0]
    raise ValueError(f"taps {taps}")


def _rows(x: torch.Tensor, r0: int, r1: int):
    """x[r0:r1] with rows outside [0, len(x)) read as zero."""
    out = torch.zeros((r1 - r0, x.shape[1]), dtype=x.dtype, device=x.device)
    a, b = max(r0, 0), min(r1, x.shape[0])
    if b > a:
        out[a - r0:b - r0] = x[a:b]
    return out


# ---- the checker --------------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound) -> tuple[float, int]:
    """Worst |got - ref| / bound (bound 0: exact) and its flat index; a NaN where ref is finite counts as infinite."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    if ref.numel() == 0:
        return 0.0, -1
    err = (got - ref).abs()
    both_nan = torch.isnan(got) & torch.isnan(ref)
    err = torch.where(both_nan, torch.zeros_like(err), torch.where(torch.isnan(err), torch.full_like(err, math.inf), err))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                    torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    i = int(torch.argmax(r.flatten()))
    return float(r.flatten()[i]), i


def check(name: str, got, ref, bound) -> float:
    """Assert the pointwise bound; returns the worst ratio."""
    w, i = ratio(got, ref, bound)
    if not w <= 1.0:
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), tuple(ref.shape)))
        raise AssertionError(f"{name}: |got - ref| / bound = {w:.3g} at {idx}: got {float(got.flatten()[i]):.9g}, "
                             f"ref {float(ref.flatten()[i]):.9g}, bound {float(bound.flatten()[i]):.3g}")
    return w


def check_planes_exact(name: str, got_hi, got_lo, exp_hi, exp_lo):
    """Split planes bit for bit, except that any NaN matches any NaN (the kernels keep the payload, torch writes 0x7fc0)."""
    for g, e, p in ((got_hi, exp_hi, "hi"), (got_lo, exp_lo, "lo")):
        g, e = g.cpu(), e.cpu()
        both_nan = torch.isnan(g.float()) & torch.isnan(e.float())
        bad = (g.view(torch.int16) != e.view(torch.int16)) & ~both_nan
        if bad.any():
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{name}: {p} plane differs at {i}: got {float(g[i]):.6g}, expected {float(e[i]):.6g}")


# ---- convolutions (conv_mfma, magnet_wgrad_ex) --------------------------------------------------------------------------------
def conv_ref(x, w, taps, wp, rows, dil=1, addend=None):
    """conv_mfma's contract in fp64: x (R, >= cin) the input rows from the kernel's input pointer (fp64, hi + lo), w (taps, cout,
    cin) fp64 (hi + lo of the pack), out[r] = sum_t w[t] x[r + off_t] (+ addend[r]) for r < rows, rows of x outside [0, R) read as
    zero (the kernel's border rows are unspecified: compare interior rows only).  Returns (ref, bound) (rows, cout)."""
    cin = w.shape[2]
    ref = torch.zeros((rows, w.shape[1]), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    for t, off in enumerate(tap_offsets(taps, wp, dil)):
        xs = _rows(x[:, :cin], off, off + rows)
        ref += xs @ w[t].T
        mag += xs.abs() @ w[t].abs().T
    if addend is not None:
        a = addend[:rows].double()
        ref += a
        mag += a.abs()
    K = taps * cin
    return ref, (1.01 * LOLO + 1.02 * gamma_l(3 * K + 2)) * mag


def wgrad_ref(dy, x, rows, wp, taps, cout, cin, dil=1):
    """magnet_wgrad_ex's contract in fp64: dW[tap][o][c] = sum over the rows whose every tap stays inside [0, rows) of
    dy[row][o] x[row + off(tap)][c]; dy, x fp64 (hi + lo).  Returns (ref, bound) laid out as nn.Conv2d's (cout, cin, k, k)."""
    offs = tap_offsets(taps, wp, dil)
    p0, p1 = -min(min(offs), 0), rows - max(max(offs), 0)
    k = {9: 3, 4: 2, 1: 1}[taps]
    ref = torch.zeros((cout, cin, k, k), dtype=torch.float64, device=dy.device)
    mag = torch.zeros_like(ref)
    d = dy[p0:p1, :cout]
    for t, off in enumerate(offs):
        xs = x[p0 + off:p1 + off, :cin]
        ref[:, :, t // k, t % k] = d.T @ xs
        mag[:, :, t // k, t % k] = d.abs().T @ xs.abs()
    P = max(p1 - p0, 0)
    L = 3 * min(P, 2048) + -(-P // 2048) + 1
    return ref, (1.01 * LOLO + 1.02 * gamma_l(L)) * mag


# ---- BatchNorm backward -------------------------------------------------------------------------------------------------------
def interior_mask(N, hp, wp, pad, device=None):
    m = torch.zeros((N, hp, wp), dtype=torch.bool, device=device)
    m[:, pad:hp - pad, pad:wp - pad] = True
    return m.reshape(-1)


def bn_backward_ref(x, grid, mean, invstd, gamma, beta, relu, g, mask=None):
    """magnet_bn_train_backward's contract.  x, g (rows, >= C) as the kernel read them; mean, invstd, gamma, beta (C).  xhat is
    computed in the dtype of x (fp32 inputs: the kernel's own fp32 xhat, two separately rounded operations).  mask (rows, C) bool:
    the forward's ReLU mask (exact); None: t = xhat gamma + beta > 0 with the marginal band of the module docstring.  Returns a
    dict of (ref, bound) pairs 'dx' (rows, C; zero with bound 0 on the border), 'dgamma', 'dbeta', and 'marginal' (a count)."""
    N, hp, wp, pad, C = (int(v) for v in grid)
    inner = interior_mask(N, hp, wp, pad, x.device)
    xi = x[:inner.numel()][inner, :C]
    xh = ((xi - mean.to(xi.dtype)) * invstd.to(xi.dtype)).double()
    gi = g[:inner.numel()][inner, :C].double()
    ga, be = gamma.double(), beta.double()
    n = xh.shape[0]
    marg = torch.zeros_like(gi, dtype=torch.bool)
    if not relu:
        m = torch.ones_like(gi, dtype=torch.bool)
    elif mask is not None:
        m = mask[:inner.numel()].to(x.device)[inner, :C]
    else:
        t = xh * ga + be
        m = t > 0
        marg = t.abs() <= 4 * U * ((xh * ga).abs() + be.abs())
    zero = torch.zeros_like(gi)
    gp = torch.where(m & ~marg, gi, zero)
    gm = torch.where(marg, gi, zero)                                       # marginal: g' is 0 or g; take the midpoint
    gpe = gp + gm / 2
    s1, s2 = gpe.sum(0), (gpe * xh).sum(0)
    d1, d2 = gm.abs().sum(0) / 2, (gm * xh).abs().sum(0) / 2                # half the spread of either choice
    a1 = (gp.abs() + gm.abs()).sum(0)
    a2 = ((gp.abs() + gm.abs()) * xh.abs()).sum(0)
    fs = n * 2.0 ** -52
    out = {"marginal": int(marg.sum())}
    out["dbeta"] = (s1, 1.01 * (U * s1.abs() + fs * a1) + d1)
    out["dgamma"] = (s2, 1.01 * (U * s2.abs() + fs * a2) + d2)
    gs = ga * invstd.double()
    dx = gs * (gpe - s1 / n - xh * s2 / n)
    b = gs.abs() * 1.01 * ((LOLO + 2 * U) * (gpe.abs() + gm.abs() / 2 + (s1 / n).abs() + (xh * s2 / n).abs())
                           + fs * (a1 / n + xh.abs() * a2 / n) + d1 / n + xh.abs() * d2 / n + gm.abs() / 2)
    rows = N * hp * wp
    ref = torch.zeros((rows, C), dtype=torch.float64, device=x.device)
    bound = torch.zeros_like(ref)
    ref[inner] = dx
    bound[inner] = b
    out["dx"] = (ref, bound)
    return out


# ---- small gathers: the feature-gradient pack and the space-to-depth backward ------------------------------------------------
def grad_pack_ref(g_nchw, pad, ld):
    """magnet_fnet_grad_pack: split_bf16 of the zero-bordered channel-last grid (N*(h+2pad)*(w+2pad), ld), channels [C, ld) zero."""
    from magnet_amd.convnet import split_bf16
    N, C, h, w = g_nchw.shape
    full = torch.zeros((N, h + 2 * pad, w + 2 * pad, ld), dtype=torch.float32, device=g_nchw.device)
    full[:, pad:pad + h, pad:pad + w, :C] = g_nchw.float().permute(0, 2, 3, 1)
    return split_bf16(full.reshape(-1, ld))


def d2s_backward_ref(g_s, N, C, H2, W2, ipad):
    """magnet_fnet_d2s_backward: (N, H2, W2, C) = the phase (y % 2) * 2 + x % 2 channels of g_s (N, H4 + 2ipad, W4 + 2ipad, 4C)
    at (y // 2, x // 2)."""
    H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
    S = g_s.double()[:N * (H4 + 2 * ipad) * (W4 + 2 * ipad)].reshape(N, H4 + 2 * ipad, W4 + 2 * ipad, 4 * C)
    S = S[:, ipad:ipad + H4, ipad:ipad + W4]
    out = torch.zeros((N, H2, W2, C), dtype=torch.float64, device=g_s.device)
    for ph, (py, px) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        ny, nx = len(range(py, H2, 2)), len(range(px, W2, 2))
        out[:, py::2, px::2] = S[:, :ny, :nx, ph * C:(ph + 1) * C]
    return out


# ---- SPP ----------------------------------------------------------------------------------------------------------------------
def bilinear_matrix(out_n, in_n, device=None):
    """(out_n, in_n) fp64 weights of the align_corners=True linear interpolation, and its two-cell support (0/1)."""
    s = (in_n - 1) / (out_n - 1) if out_n > 1 else 0.0
    f = torch.arange(out_n, dtype=torch.float64, device=device) * s
    i0 = f.floor().clamp(max=in_n - 1).long()
    i1 = (i0 + 1).clamp(max=in_n - 1)
    l1 = f - i0
    W = torch.zeros((out_n, in_n), dtype=torch.float64, device=device)
    o = torch.arange(out_n, device=device)
    W.index_put_((o, i0), 1.0 - l1, accumulate=True)
    W.index_put_((o, i1), l1, accumulate=True)
    cells = torch.arange(in_n, dtype=torch.float64, device=device)
    S = ((f[:, None] - cells[None, :]).abs() < 1.0 + 1e-6).double()
    return W, S


def spp_upsample_bwd_ref(g, c_off, N, h, w, pad, ph, pw):
    """magnet_spp_upsample_backward: the fp64 gradient of the (N, 32, ph, pw) -> (h, w) align_corners bilinear upsampling for the
    output gradient g (interior of the bordered (N, h+2pad, w+2pad, g_ld) grid, channels [c_off, c_off + 32)).  (ref, bound) as
    (N*ph*pw, 32)."""
    G = g.double()[:N * (h + 2 * pad) * (w + 2 * pad)].reshape(N, h + 2 * pad, w + 2 * pad, -1)
    G = G[:, pad:pad + h, pad:pad + w, c_off:c_off + 32]
    Wy, Sy = bilinear_matrix(h, ph, g.device)
    Wx, Sx = bilinear_matrix(w, pw, g.device)
    ref = torch.einsum("yi,nyxc,xj->nijc", Wy, G, Wx).reshape(-1, 32)
    mag = torch.einsum("yi,nyxc,xj->nijc", Wy, G.abs(), Wx).reshape(-1, 32)
    sup = torch.einsum("yi,nyxc,xj->nijc", Sy, G.abs(), Sx).reshape(-1, 32)
    Lx = min(w, 2 * (w - 1) // max(pw - 1, 1) + 4)
    Ly = min(h, 2 * (h - 1) // max(ph - 1, 1) + 4)
    L = Lx + -(-Ly // 8) + 12
    ey, ex = 4 * U * (ph + 1), 4 * U * (pw + 1)
    return ref, 1.01 * gamma_l(L) * mag + (ey + ex + ey * ex) * sup


def spp_pool_bwd_ref(g, c_off, N, h, w, pad, dpools, ks=(64, 32, 16, 8)):
    """magnet_spp_pool_backward: g channels [c_off, c_off + 128) + the AvgPool2d(k, k) backward of each branch's dpool
    (N*(h//k)*(w//k), 128) over the interior.  (ref, bound) as (N, h, w, 128)."""
    G = g.double()[:N * (h + 2 * pad) * (w + 2 * pad)].reshape(N, h + 2 * pad, w + 2 * pad, -1)
    G = G[:, pad:pad + h, pad:pad + w, c_off:c_off + 128]
    ref, terms = G.clone(), torch.zeros_like(G)
    cover = torch.zeros((N, h, w, 1), dtype=torch.bool, device=g.device)
    for k, d in zip(ks, dpools):
        ph, pw = h // k, w // k
        up = (d.double().reshape(N, ph, pw, 128) / (k * k)).repeat_interleave(k, 1).repeat_interleave(k, 2)
        ref[:, :ph * k, :pw * k] += up
        terms[:, :ph * k, :pw * k] += up.abs()
        cover[:, :ph * k, :pw * k] = True
    return ref, 8 * U * 1.01 * (terms + G.abs() * cover)


# ---- the stem's weight gradient ----------------------------------------------------------------------------------------------
def stem_wgrad_ref(img, dz):
    """magnet_fnet_stem_wgrad: the weight gradient of the 3 -> 32 3x3 stride-2 pad-1 convolution of the fp32 image (N, 3, H, W)
    for dz = (hi, lo) split planes of the (N, H2+2, W2+2, 32) grid.  (ref, bound) as (32, 3, 3, 3)."""
    N, _, H, W = img.shape
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    D = join(*dz)[:N * (H2 + 2) * (W2 + 2)].reshape(N, H2 + 2, W2 + 2, 32)[:, 1:-1, 1:-1].reshape(N, H2 * W2, 32)
    cols = F.unfold(img.double(), 3, padding=1, stride=2)                 # (N, 27, H2*W2), row ci*9 + dy*3 + dx
    ref = torch.einsum("nkp,npo->ok", cols, D).reshape(32, 3, 3, 3)
    mag = torch.einsum("nkp,npo->ok", cols.abs(), D.abs()).reshape(32, 3, 3, 3)
    P = N * H2 * W2
    L = -(-P // 256) + 1
    return ref, ((L + 1) * U + U) * 1.01 * mag
