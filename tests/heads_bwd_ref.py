"""fp64 restatements of the G-Net / mask-head training backward's launches (magnet_amd/train.py, csrc/train_bwd.hip): the Gaussian NLL
forward and backward, the convex-upsampling backward, the three stages of the 1x1-tail dgrad and the weight / bias gradient.  Each
takes exactly what the kernel received, works in float64 on the device of its inputs, and returns (ref, bound) pairs for the checker
of tests/fnet_bwd_ref.py (|got - ref| <= bound everywhere; a bound of 0 means bit-exact).  Notation as there: u = 2^-24, gamma_L the
cost of a chain of L fp32 roundings, LOLO = 2^-16 the dropped lo lo of a bf16x3 product and the residual of a hi + lo split.

  nll_forward          per pixel the kernel forms t = d^2 / (2 var) + 0.5 logf(var) in fp32 (d = mu - gt, var = sigma^2 clamped to
                       1e-10f where sigma^2 < 1e-10f, that decision taken on the fp32 square exactly as the kernel takes it):
                       d^2 / (2 var) carries <= gamma_5 (d, d^2, var, the division), logf <= 2 ulp of its value plus the 1.01 u its
                       argument's rounding moves it, the final addition u: e <= gamma_7 |A| + 5.1 u |B| + 0.51 u, A = d^2/(2var),
                       B = 0.5 log var.  The sums are fp64 (per thread ceil(P / 65536) additions, an 8-level tree, then 256 blocks in
                       order): + (ceil(P / 65536) + 264) 2^-53 sum |t|.  The count is exact.  loss = sum_i gamma^(n-1-i) S_i / count
                       in fp64, stored as fp32: sum_i gamma^(n-1-i) bound_i / count + 1.01 u |loss|.
  nll_backward         scale = grad_loss gamma^(n-1-i) / count rounded to fp32 (u); gmu = scale (d / var): gamma_6 |gmu|; gsig =
                       scale ((0.5 / var - d^2 / (2 var^2)) 2 sigma): the difference may cancel, so gamma_10 |scale| (0.5 / var +
                       d^2 / (2 var^2)) 2 |sigma|.  Bit-exact 0 where the pixel is masked; gsig bit-exact 0 where var is clamped.
  upsample_backward    p = softmax of the 9 logits in fp32: expf of the rounded x = l - max costs u |x| + 2u, the sum of 9 terms
                       gamma_9, the division u: |dp_t| <= 1.01 p_t (eps_t + sum_s p_s eps_s + gamma_9 + u) + 2^-120 (eps = u (|x| +
                       2); the last term covers an exp that underflows).  G_t = sum over the n iterations and 2 channels of g D_t:
                       gamma_(2n+1).  d mask = p_t (G_t - sum_s p_s G_s): the p and G errors propagated, gamma_10 for the inner
                       product, u for the difference and the product.  part = sum over the k^2 sub-pixels of p g: gamma_(k^2+1);
                       d depth = up to 9 parts in tap order: gamma_9.
  head_dgrad           first stage: the dout form splits dout on every row below rows (bit-exact); the G-Net form computes
                       d mu_1 = d mu s0 (u) and d sigma_1 = d sigma elu'(o1) s0 (expf <= 2 ulp, two products: gamma_5) on interior
                       rows and 0 on border rows, and its written planes add the split (LOLO).  Each transposed product is
                       restated from the operand the kernel held (hi + lo it wrote): (1.01 LOLO + 1.02 gamma_(3K+1)) |W^T| |g| for
                       the fp32 value (acc), + LOLO of it for the written planes.  Mask [h_hi > 0] on the bf16 plane the kernel
                       read; a positive subnormal h_hi is marginal (a flush-to-zero compare reads it as 0): either choice is
                       accepted there (midpoint, half the spread).  Border rows: bit-exact 0.  acc_mode 2: + u |acc_old + dh1|.
  wgrad                rows [wp + 1, rows - wp - 1) in chunks of 2048: (1.01 LOLO + 1.02 gamma_(3 min(P, 2048) + nchunks + 1))
                       sum |dy| |x| for the weights; the bias is summed by 16 lanes over ceil(chunk / 16) rows each (hi + lo
                       added first), then the 16 lane sums, then the chunks in order: gamma_(ceil(min(P, 2048) / 16) + 17 +
                       nchunks) sum |dy|.  accumulate: + 1.01 u |old + sum|.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from magnet_amd.convnet import split_bf16
from tests.fnet_bwd_ref import LOLO, U, check, check_planes_exact, gamma_l, interior_mask, join, ratio  # noqa: F401

CLAMP = float(torch.tensor(1e-10, dtype=torch.float32))   # the clamp constant as the kernel holds it (1e-10f)
WG_CHUNK = 2048
NLL_THREADS = 256 * 256


# ---- Gaussian NLL ---------------------------------------------------------------------------------------------------------------
def _nll_terms(preds, gt, mask):
    p = preds.float()
    sig32 = p[:, :, 1]
    clamped = (sig32 * sig32) < CLAMP                                   # the kernel's decision, on the fp32 square
    P = preds.double()
    mu, sg = P[:, :, 0], P[:, :, 1]
    var = torch.where(clamped, torch.full_like(sg, CLAMP), sg * sg)
    d = mu - gt.double()[None]
    return d, var, sg, clamped, mask.bool()[None].expand_as(d)


def nll_forward_ref(preds, gt, mask, gamma):
    """magnet_nll_loss_forward: preds (n, B, 2, H, W), gt (B, H, W), mask (B, H, W).  Returns {'count': exact fp64, 'sums': (ref,
    bound) (n,), 'loss': (ref, bound) 0-d}."""
    d, var, _, _, m = _nll_terms(preds, gt, mask)
    n = d.shape[0]
    A = d * d / (2 * var)
    Bt = 0.5 * torch.log(var)
    t = torch.where(m, A + Bt, torch.zeros_like(A))
    e = torch.where(m, gamma_l(7) * A.abs() + 5.1 * U * Bt.abs() + 0.51 * U, torch.zeros_like(A))
    npix = mask.numel()
    L64 = -(-npix // NLL_THREADS) + 264
    sums = t.flatten(1).sum(1)
    sb = e.flatten(1).sum(1) + 1.01 * L64 * 2.0 ** -53 * t.abs().flatten(1).sum(1)
    count = mask.bool().sum().double()
    w = torch.tensor([gamma ** (n - 1 - i) for i in range(n)], dtype=torch.float64, device=sums.device)
    loss = (w * sums / count).sum()
    lb = (w * sb / count).sum() + 1.01 * U * loss.abs() + 1e-14 * (w * sums.abs() / count).sum()
    return {"count": count, "sums": (sums, sb), "loss": (loss, lb)}


def nll_backward_ref(preds, gt, mask, count, grad_loss, gamma):
    """magnet_nll_loss_backward: (ref, bound) of grad_preds (n, B, 2, H, W) for the device scalar grad_loss and the count the
    forward wrote."""
    d, var, sg, clamped, m = _nll_terms(preds, gt, mask)
    n = d.shape[0]
    w = torch.tensor([gamma ** (n - 1 - i) for i in range(n)], dtype=torch.float64, device=d.device)
    scale = (float(grad_loss) * w / float(count)).reshape(n, 1, 1, 1)
    zero = torch.zeros_like(d)
    gmu = torch.where(m, scale * d / var, zero)
    bmu = gamma_l(6) * gmu.abs()
    a, b = 0.5 / var, d * d / (2 * var * var)
    live = m & ~clamped
    gsig = torch.where(live, scale * (a - b) * 2 * sg, zero)
    bsig = torch.where(live, gamma_l(10) * scale.abs() * (a + b) * 2 * sg.abs(), zero)
    return torch.stack([gmu, gsig], 2), torch.stack([bmu, bsig], 2)


# ---- convex-upsampling backward -------------------------------------------------------------------------------------------------
def strided(buf, layout, shape):
    """The (B, C, h, w) view of a flat fp32 buffer addressed by layout = (element offset, sb, sc, sy, sx)."""
    o, sb, sc, sy, sx = layout
    return buf.as_strided(shape, (sb, sc, sy, sx), buf.storage_offset() + o)


def addressed(buf, layout, shape):
    """bool like buf: True at the elements `layout` addresses."""
    m = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    strided(m, layout, shape).fill_(True)
    return m


def _taps():
    return [(t // 3 - 1, t % 3 - 1) for t in range(9)]


def upsample_bwd_ref(gup, depth, mask, k, mask_layout=None):
    """magnet_upsample_depth_backward: gup (n, B, 2, kh, kw), depth (n, B, 2, h, w), mask NCHW (B, 9k^2, h, w) or a flat buffer
    addressed by mask_layout.  Returns {'grad_depth': (ref, bound) like depth, 'grad_mask': (ref, bound) (B, 9k^2, h, w)}."""
    n, B, _, h, w = depth.shape
    kk = k * k
    lg = mask if mask_layout is None else strided(mask, mask_layout, (B, 9 * kk, h, w))
    Lg = lg.double().reshape(B, 9, kk, h, w)
    x = Lg - Lg.amax(1, keepdim=True)
    p = torch.softmax(x, 1)
    eps = U * (x.abs() + 2)
    prel = eps + (p * eps).sum(1, keepdim=True) + gamma_l(9) + U
    perr = 1.01 * p * prel + 2.0 ** -120
    Dp = F.pad(depth.double(), (1, 1, 1, 1))
    Dt = torch.stack([Dp[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy, dx in _taps()], 3)          # (n, B, 2, 9, h, w)
    g = gup.double().reshape(n, B, 2, h, k, w, k).permute(0, 1, 2, 4, 6, 3, 5).reshape(n, B, 2, kk, h, w)
    G = torch.einsum("nbcsyx,nbctyx->btsyx", g, Dt)
    Gerr = gamma_l(2 * n + 1) * torch.einsum("nbcsyx,nbctyx->btsyx", g.abs(), Dt.abs())
    pG = (p * G).sum(1, keepdim=True)
    pGerr = (perr * G.abs() + p * Gerr).sum(1, keepdim=True) + gamma_l(10) * (p * G.abs()).sum(1, keepdim=True)
    diff = G - pG
    gm = p * diff
    gmb = 1.01 * (perr * diff.abs() + p * (Gerr + pGerr + U * diff.abs()) + U * gm.abs())
    part = torch.einsum("btsyx,nbcsyx->nbctyx", p, g)
    perr_part = torch.einsum("btsyx,nbcsyx->nbctyx", perr, g.abs()) + gamma_l(kk + 1) * torch.einsum("btsyx,nbcsyx->nbctyx", p, g.abs())
    pp, pe, pa = (F.pad(v, (1, 1, 1, 1)) for v in (part, perr_part, part.abs()))
    gd = torch.zeros_like(depth, dtype=torch.float64)
    gdb = torch.zeros_like(gd)
    for t, (dy, dx) in enumerate(_taps()):
        sl = (Ellipsis, t, slice(1 - dy, 1 - dy + h), slice(1 - dx, 1 - dx + w))
        gd += pp[sl]
        gdb += pe[sl] + gamma_l(9) * pa[sl]
    return {"grad_depth": (gd, gdb), "grad_mask": (gm.reshape(B, 9 * kk, h, w), gmb.reshape(B, 9 * kk, h, w))}


# ---- head dgrad -----------------------------------------------------------------------------------------------------------------
def wt_parts(wt, k0):
    """The flat [W4^T (128, k0) | W3^T (128, 128) | W2^T (128, 128)] weight operand (fp64) -> its three matrices."""
    v = wt.double().reshape(-1)
    return v[:128 * k0].reshape(128, k0), v[128 * k0:128 * k0 + 16384].reshape(128, 128), v[128 * k0 + 16384:].reshape(128, 128)


def gauss_stage_ref(grad_gmm, gnet_out, gmm_in, B, h, w, elu_prime=None):
    """G-Net form of the first stage: (ref, bound) (rows, 32) of the value the kernel splits into dout_hi / dout_lo, the bound
    including that split.  elu_prime: a replacement for the derivative (planted-defect tests only)."""
    rows = B * (h + 2) * (w + 2)
    dev = grad_gmm.device
    inner = interior_mask(B, h + 2, w + 2, 1, dev)
    gg, s0 = grad_gmm.double(), gmm_in.double()[:, 1].reshape(-1)
    o1 = gnet_out[:rows][inner, 1].double()
    el = torch.where(o1 > 0, torch.ones_like(o1), torch.exp(o1)) if elu_prime is None else elu_prime(o1)
    ref = torch.zeros((rows, 32), dtype=torch.float64, device=dev)
    b = torch.zeros_like(ref)
    ref[inner, 0] = gg[:, 0].reshape(-1) * s0
    ref[inner, 1] = gg[:, 1].reshape(-1) * el * s0
    b[inner, 0] = U * ref[inner, 0].abs()
    b[inner, 1] = gamma_l(5) * ref[inner, 1].abs()
    return ref, b + LOLO * (ref.abs() + b)


def dgrad_stage_ref(wt, g, h_hi, B, h, w):
    """One transposed product of magnet_head_dgrad: [h_hi > 0] (g @ wt^T) on interior rows, 0 on border rows.  wt (128, K) fp64,
    g (rows, K) the operand the kernel multiplied (hi + lo), h_hi the bf16 plane the kernel read.  Returns {'acc': (ref, bound) of
    the fp32 value, 'planes': (ref, bound) of the split planes it writes, 'marginal': count}."""
    rows, K = g.shape
    inner = interior_mask(B, h + 2, w + 2, 1, g.device)[:rows, None]
    y = g.double() @ wt.double().T
    mag = g.double().abs() @ wt.double().abs().T
    hv = h_hi[:rows].float()
    on = (hv > 0) & inner
    marg = on & (hv < 2.0 ** -126)
    zero = torch.zeros_like(y)
    ref = torch.where(on & ~marg, y, zero) + torch.where(marg, y / 2, zero)
    b = torch.where(on, (1.01 * LOLO + 1.02 * gamma_l(3 * K + 1)) * mag, zero) + torch.where(marg, y.abs() / 2, zero)
    return {"acc": (ref, b), "planes": (ref, b + LOLO * (ref.abs() + b)), "marginal": int(marg.sum())}


def acc_ref(stage, acc_old, mode):
    """The fp32 acc after a launch with acc_mode 1 (acc = dh1) or 2 (acc += dh1): (ref, bound)."""
    ref, b = stage["acc"]
    if mode == 1:
        return ref, b
    tot = acc_old.double() + ref
    return tot, b + 1.01 * U * (tot.abs() + b)


def check_head_dgrad(name, B, h, w, k0, wt, hs, outs, dout=None, gauss=None, sentinel=3.0):
    """The three stages of one launch against their restatements (each from the planes the kernel wrote) and the sentinel rows;
    wt = (hi, lo) flat weight planes, hs = [h1_hi, h2_hi, h3_hi], outs = (dout, dh3, dh2, dh1) as (hi, lo) pairs; rows past the
    grid must still hold `sentinel` (None: not checked).  Returns (worst ratio, the dh1 stage for acc checks, marginal count)."""
    rows = B * (h + 2) * (w + 2)
    dp, d3, d2, d1 = outs
    W4T, W3T, W2T = wt_parts(join(*wt), k0)
    if dout is not None:
        eh, el = split_bf16(dout[:rows].float())
        check_planes_exact(f"{name} dout planes", dp[0][:rows], dp[1][:rows], eh, el)
        worst = 0.0
    else:
        worst = check(f"{name} dout planes", join(*dp)[:rows], *gauss_stage_ref(*gauss, B, h, w))
    marg = 0
    s = None
    for st, g, hh, o in (("dh3", dp, hs[2], d3), ("dh2", d3, hs[1], d2), ("dh1", d2, hs[0], d1)):
        s = dgrad_stage_ref(W4T if st == "dh3" else (W3T if st == "dh2" else W2T), join(*g)[:rows], hh, B, h, w)
        worst = max(worst, check(f"{name} {st}", join(*o)[:rows], *s["planes"]))
        marg += s["marginal"]
    for t in (*dp, *d3, *d2, *d1):
        assert sentinel is None or (t[rows:].float() == sentinel).all(), f"{name}: a row past the grid was written"
    return worst, s, marg


# ---- weight gradient ------------------------------------------------------------------------------------------------------------
def wgrad_chunks(rows, wp):
    P = max(rows - 2 * wp - 2, 0)
    return P, -(-P // WG_CHUNK)


def wgrad_plain_ref(dy, x, rows, wp, taps, cout, cin, cout_valid=None, cin_valid=None, old_w=None, old_b=None):
    """magnet_wgrad: dW[o][c][tap] = sum over rows [wp + 1, rows - wp - 1) of dy[row][o] x[row + off(tap)][c] for o < cout_valid,
    c < cin_valid (nn.Conv2d's (cout, cin, k, k)), db[o] = sum dy[row][o]; dy, x fp64 (hi + lo).  old_w / old_b: what accumulate
    adds to.  Returns {'w': (ref, bound), 'b': (ref, bound)}."""
    cv = cout if cout_valid is None else cout_valid
    ci = cin if cin_valid is None else cin_valid
    k = 3 if taps == 9 else 1
    offs = [(t // 3 - 1) * wp + (t % 3 - 1) for t in range(9)] if taps == 9 else [0]
    p0, p1 = wp + 1, rows - wp - 1
    P, nch = wgrad_chunks(rows, wp)
    d = dy[p0:p1, :cv].double()
    ref = torch.zeros((cv, ci, k, k), dtype=torch.float64, device=dy.device)
    mag = torch.zeros_like(ref)
    for t, off in enumerate(offs):
        xs = x[p0 + off:p1 + off, :ci].double()
        ref[:, :, t // k, t % k] = d.T @ xs
        mag[:, :, t // k, t % k] = d.abs().T @ xs.abs()
    bw = (1.01 * LOLO + 1.02 * gamma_l(3 * min(P, WG_CHUNK) + nch + 1)) * mag
    rb, bb = d.sum(0), gamma_l(-(-min(P, WG_CHUNK) // 16) + 17 + nch) * d.abs().sum(0)
    if old_w is not None:
        ref = ref + old_w.double()
        bw = bw + 1.01 * U * (ref.abs() + bw)
    if old_b is not None:
        rb = rb + old_b.double()
        bb = bb + 1.01 * U * (rb.abs() + bb)
    return {"w": (ref, bw), "b": (rb, bb)}


def check_untouched(name, buf, keep, sentinel):
    """Every element of buf outside the bool `keep` still holds `sentinel` (NaN: still NaN)."""
    rest = buf[~keep]
    ok = torch.isnan(rest) if isinstance(sentinel, float) and math.isnan(sentinel) else rest == sentinel
    if not bool(ok.all()):
        raise AssertionError(f"{name}: {int((~ok).sum())} elements outside the written region changed")
