"""fp64 restatement of DnetLoss (magnet_amd/losses.py, csrc/dnet_loss.hip; the reference's upsample_depth_via_mask + activation_G +
DnetLoss, D_dense_depth.py:86-100, DNET.py:56-60, utils/losses.py:8-24) in both forms, with pointwise error bounds derived from the
kernels' own arithmetic, and an fp32 numpy emulation of the kernels in their operation order.

The restatement, per fine pixel (4y+i, 4x+j) over the 9 taps t (logit channel t*16 + i*4 + j, o_ct = depth[c](y+dy_t, x+dx_t), zero outside):
  m = max_t l_t, a_t = m - l_t >= 0, e_t = exp(-a_t), Z = sum e_t, w_t = e_t / Z;  mu = sum w_t o_0t, vu = sum w_t o_1t;
  var = elu(vu) + 1 + 1e-10;  d = mu - gt;  nll = d^2 / (2 var) + 0.5 log var;  loss = mean over valid.
  c = grad_loss / count;  g_mu = c d / var;  h = 0.5 / var - d^2 / (2 var^2);  g_v = c h elu'(vu), elu' = 1 (vu > 0) or exp(vu);
  G_t = g_mu o_0t + g_v o_1t;  grad_mask_t = w_t (G_t - sum_u w_u G_u);  grad_depth[c](q) = sum_t sum_ij (w_t g_c)(q - off_t; i, j).

Bounds.  u = 2^-24; expf, expm1f, logf within 2 ulp = 4 u relative; +, *, / correctly rounded (u each); no fused multiply-add.
Weights.  e^_t = expf(fl(l_t - m)): the subtraction's rounding moves the exponent by a_t u, so e^_t = e_t (1 +- (4 + a_t) u).  den sums
  9 positive terms in order (8 roundings): den^ = Z (1 +- Kz u) with Kz = 12 + sum w_t a_t (the weighted mean of the terms' errors).
  inv = fl(1 / den^) (u), w^_t = fl(e^_t inv) (u):  w^_t = w_t (1 +- r_t u),  r_t = Kz + a_t + 6.  An e_t below the normal range may lose
  all its bits: an absolute TINY = 2^-126 on w_t (inv <= 1), which every bound below carries as a TINY term.
Upsampling.  acc += fl(w^_t o_t): the product (u) and at most 8 roundings of a partial sum that is at most sum w |o|:
  |up^ - up| <= 1.01 u sum_t w_t |o_t| (r_t + 9) + 2 TINY sum |o_t|                                                (b_mu, b_vu)
  (1.01 absorbs the second-order terms throughout).
Variance.  elu is 1-Lipschitz and expm1f is within 4 u of it; (elu + 1) and (.. + 1e-10) round once each, fl32(1e-10) is within u:
  |var^ - var| <= 1.01 (b_vu + u (4 |elu| + |elu + 1| + 2 var))                                                     (b_var)
  This is ABSOLUTE and of the order of u, while var itself goes down to 1e-10 when vu is below about -17: there the fp32 arithmetic
  (the kernel's and torch's alike) cannot tell var from its floor, and every bound that divides by var is accordingly wide.  The
  kernel's var is never below fl32(1e-10) (a sum of non-negative terms, monotonic rounding), so the box of variances the bounds range
  over is [vlo, var + b_var], vlo = min(var, max(var - b_var, fl32(1e-10))).
NLL and the gradients with respect to (mu, var) are smooth functions of (d, var) on the box |d'| <= Dm = |d| + b_d, var' >= vlo, with
b_d = b_mu + u |d| (the subtraction).  Mean value theorem with the partial derivatives bounded over the box, plus the roundings of the
kernel's own operations at their largest magnitudes over the box:
  nll:  |d/dd| <= Dm / vlo, |d/dvar| <= 0.5 / vlo + Dm^2 / (2 vlo^2); roundings d*d, /(2 var) (2 var is exact), logf (4 u), the sum:
        b_nll = 1.01 [Dm / vlo b_d + (0.5 / vlo + Dm^2 / (2 vlo^2)) b_var + u (4 Dm^2 / (2 vlo) + 5 * 0.5 max|log var'|)]
  g_mu = c d / var:  b_gmu = 1.01 |c| [b_d / vlo + Dm / vlo^2 b_var + 4 u Dm / vlo]      (c = fl32(grad_loss / count), the quotient, the product)
  h:    |dh/dd| <= Dm / vlo^2, |dh/dvar| <= 0.5 / vlo^2 + Dm^2 / vlo^3; roundings 0.5 / var, d*d, var*var, the quotient, the difference:
        b_h = Dm / vlo^2 b_d + (0.5 / vlo^2 + Dm^2 / vlo^3) b_var + u (2 * 0.5 / vlo + 5 Dm^2 / (2 vlo^2)),   |h'| <= Hs = 0.5 / vlo + Dm^2 / (2 vlo^2)
  elu' = min(1, exp(vu)) is 1-Lipschitz (so a vu^ on the other side of 0 costs no more than b_vu), expf 4 u: b_de = b_vu + 5 u elu'
  g_v = (c h) elu':  b_gv = 1.01 |c| [b_h de_s + Hs b_de + 4 u Hs de_s],  de_s = min(1, elu' + b_de)
  loss: the mean of b_nll over the valid pixels + (u + n 2^-52) mean |nll| (the fp64 sum of n terms, the fp32 result).  The count is exact.
Mask gradient.  G^_t = fl(fl(g_mu o_0t) + fl(g_v o_1t)):  b_G = b_gmu |o_0t| + b_gv |o_1t| + 2 u (|g_mu|' |o_0t| + |g_v|' |o_1t|) (' = the value
  plus its bound);  S^ = sum_u fl(w^_u G^_u) in order:  b_S = sum_u w_u [b_G_u + u (r_u + 9) |G_u|'];  fl(w^_t fl(G^_t - S^)):
        b_gmask = 1.01 w_t [b_G_t + b_S + u (r_t + 2) |G_t - S|] + TINY (1 + |G_t|' + |S|')
Depth gradient.  Every term fl(w^_t g^_c) carries w_t b_g + u w_t (r_t + 1) |g|'; the 16 sub-pixel terms of a (pixel, tap) are added in a
  fixed order (15 roundings) and the 9 taps gathered in order (8 roundings), all bounded by the sum of the terms' magnitudes:
        b_gdepth = 1.01 sum_t sum_ij w_t [b_g + u (r_t + 24) |g|'] gathered like the gradient itself, + 144 TINY
Plain form (pred = [mu, var] given): the same with b_mu = 0, b_var = 0, except at a clamped pixel (var < 1e-10), where var is the
constant 1e-10 (fl32: within u) and the var gradient is exactly zero.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126
F32_FLOOR = float(np.float32(1e-10))


def to_sub(x):
    """(B, 4h, 4w) -> (B, 4, 4, h, w) [b, i, j, y, x]."""
    B, H, W = x.shape
    return x.reshape(B, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3)


def to_fine(x):
    """(B, 4, 4, h, w) [b, i, j, y, x] -> (B, 4h, 4w)."""
    B, _, _, h, w = x.shape
    return x.permute(0, 3, 1, 4, 2).reshape(B, 4 * h, 4 * w)


def _patches(depth):
    """(B, 2, h, w) -> (B, 2, 9, h, w): the 3x3 neighbourhood in unfold order, zero outside."""
    B, C, h, w = depth.shape
    return F.unfold(depth, [3, 3], padding=1).reshape(B, C, 9, h, w)


def _gather(part, flip=False):
    """(B, 2, 9, h, w) per-(pixel, tap) sums -> (B, 2, h, w): out(q) = sum_t part_t(q - off_t), the adjoint of _patches.
    flip: the sign of the offset reversed (a negative control)."""
    B, C, _, h, w = part.shape
    if flip:
        part = part.flip(2)
    return F.fold(part.reshape(B, C * 9, h * w), (h, w), [3, 3], padding=1)


def _nll_terms(d, bd, var, bvar, vlo, c):
    """nll, g_mu, h (the var gradient before c and elu') of (d, var) with their bounds over the box |d'| <= |d| + bd, var' >= vlo."""
    Dm = d.abs() + bd
    nll = d * d / (2 * var) + 0.5 * torch.log(var)
    logs = torch.maximum(torch.log(vlo).abs(), torch.log(var + bvar).abs())
    b_nll = 1.01 * (Dm / vlo * bd + (0.5 / vlo + Dm * Dm / (2 * vlo * vlo)) * bvar + U * (4 * Dm * Dm / (2 * vlo) + 2.5 * logs))
    gm = c * d / var
    b_gm = 1.01 * abs(c) * (bd / vlo + Dm / (vlo * vlo) * bvar + 4 * U * Dm / vlo)
    h = 0.5 / var - d * d / (2 * var * var)
    A1, A2 = 0.5 / vlo, Dm * Dm / (2 * vlo * vlo)
    b_h = Dm / (vlo * vlo) * bd + (0.5 / (vlo * vlo) + Dm * Dm / vlo ** 3) * bvar + U * (2 * A1 + 5 * A2)
    return nll, b_nll, gm, b_gm, h, b_h, A1 + A2


def _mean(nll, b_nll, valid):
    n = int(valid.sum())
    if not n:
        return n, float("nan"), 0.0
    loss = float(nll[valid].sum() / n)
    return n, loss, float(b_nll[valid].sum() / n) + (U + n * 2.0 ** -52) * float(nll[valid].abs().sum() / n)


def dnet_loss_ref(depth, mask, gt, valid, grad_loss=1.0, elu_grad_one=False, flip_offsets=False):
    """depth (B,2,h,w), mask (B,144,h,w), gt (B,4h,4w), valid (B,4h,4w) bool: everything in float64 on depth's device.  Returns a dict:
    pred (B,2,4h,4w) [mu, var], loss, count, grad_depth (B,2,h,w), grad_mask (B,144,h,w) and bound_* of each.
    elu_grad_one / flip_offsets: two deliberately wrong gradients (negative controls of the bounds)."""
    depth = depth.detach().double()
    B, _, h, w = depth.shape
    L = mask.detach().double().to(depth.device).reshape(B, 9, 4, 4, h, w)
    g = to_sub(gt.detach().double().to(depth.device))
    va = to_sub(valid.detach().to(depth.device).bool())
    m = L.amax(dim=1, keepdim=True)
    a = m - L
    e = torch.exp(-a)
    p = e / e.sum(dim=1, keepdim=True)
    P = _patches(depth)
    o0, o1 = P[:, 0].reshape(B, 9, 1, 1, h, w), P[:, 1].reshape(B, 9, 1, 1, h, w)
    mu, vu = (p * o0).sum(1), (p * o1).sum(1)                                # (B, 4, 4, h, w)
    pa = torch.where(p > 0, p * a, torch.zeros_like(p))                       # p = 0 where a is huge: the term is 0
    Kz = 12 + pa.sum(1, keepdim=True)
    prw = p * (Kz + 6) + pa                                                   # w_t r_t
    b_mu = 1.01 * U * ((prw + 9 * p) * o0.abs()).sum(1) + 2 * TINY * o0.abs().sum(1)
    b_vu = 1.01 * U * ((prw + 9 * p) * o1.abs()).sum(1) + 2 * TINY * o1.abs().sum(1)
    elu = torch.where(vu > 0, vu, torch.expm1(vu))
    var = elu + 1 + 1e-10
    b_var = 1.01 * (b_vu + U * (4 * elu.abs() + (elu + 1).abs() + 2 * var))
    vlo = torch.minimum(var, torch.clamp(var - b_var, min=F32_FLOOR))
    out = dict(pred=torch.stack([to_fine(mu), to_fine(var)], 1), bound_pred=torch.stack([to_fine(b_mu), to_fine(b_var)], 1))

    n = int(va.sum())
    c = float(grad_loss) / n if n else 0.0
    d = mu - g
    bd = b_mu + U * d.abs()
    nll, b_nll, gm, b_gm, hh, b_h, Hs = _nll_terms(d, bd, var, b_var, vlo, c)
    _, out["loss"], out["bound_loss"] = _mean(nll, b_nll, va)
    out["count"] = n

    de = torch.ones_like(vu) if elu_grad_one else torch.where(vu > 0, torch.ones_like(vu), torch.exp(vu))
    b_de = b_vu + 5 * U * de
    des = torch.clamp(de + b_de, max=1.0)
    gv = c * hh * de
    b_gv = 1.01 * abs(c) * (b_h * des + Hs * b_de + 4 * U * Hs * des)
    zero = torch.zeros_like(gm)
    gm, b_gm, gv, b_gv = (torch.where(va, t, zero) for t in (gm, b_gm, gv, b_gv))
    gm_, bgm_, gv_, bgv_ = (t.unsqueeze(1) for t in (gm, b_gm, gv, b_gv))
    gms, gvs = gm_.abs() + bgm_, gv_.abs() + bgv_
    G = gm_ * o0 + gv_ * o1                                                   # (B, 9, 4, 4, h, w)
    b_G = bgm_ * o0.abs() + bgv_ * o1.abs() + 2 * U * (gms * o0.abs() + gvs * o1.abs())
    Gs = G.abs() + b_G
    S = (p * G).sum(1, keepdim=True)
    b_S = (p * b_G).sum(1, keepdim=True) + U * ((prw + 9 * p) * Gs).sum(1, keepdim=True)
    gmask = p * (G - S)
    b_gmask = 1.01 * (p * (b_G + b_S) + U * (prw + 2 * p) * (G - S).abs()) + TINY * (1 + Gs + S.abs() + b_S)
    out["grad_mask"], out["bound_grad_mask"] = gmask.reshape(B, 144, h, w), b_gmask.reshape(B, 144, h, w)

    part = torch.stack([(p * gm_).sum((2, 3)), (p * gv_).sum((2, 3))], 1)     # (B, 2, 9, h, w)
    b_part = torch.stack([(p * bgm_ + U * (prw + 24 * p) * gms).sum((2, 3)), (p * bgv_ + U * (prw + 24 * p) * gvs).sum((2, 3))], 1)
    out["grad_depth"] = _gather(part, flip=flip_offsets)
    out["bound_grad_depth"] = 1.01 * _gather(b_part) + 144 * TINY
    return out


def dnet_nll_ref(pred, gt, valid, grad_loss=1.0):
    """The plain form in float64: pred (B,2,H,W) [mu, var] (fp32 values), gt (B,H,W), valid (B,H,W) bool.  Returns loss, count, grad
    (B,2,H,W), clamped (B,H,W) bool and bound_loss, bound_grad."""
    clamped = pred.detach()[:, 1].float() < np.float32(1e-10)                  # the kernel's comparison, in fp32
    pr = pred.detach().double()
    mu, var0 = pr[:, 0], pr[:, 1]
    var = torch.where(clamped, torch.full_like(var0, 1e-10), var0)
    b_var = torch.where(clamped, U * var, torch.zeros_like(var))
    va = valid.detach().bool().to(pr.device)
    n = int(va.sum())
    c = float(grad_loss) / n if n else 0.0
    d = mu - gt.detach().double().to(pr.device)
    nll, b_nll, gm, b_gm, hh, b_h, Hs = _nll_terms(d, U * d.abs(), var, b_var, var - b_var, c)
    _, loss, bound_loss = _mean(nll, b_nll, va)
    zero = torch.zeros_like(gm)
    gv = torch.where(va & ~clamped, c * hh, zero)
    b_gv = torch.where(va & ~clamped, 1.01 * abs(c) * (b_h + 4 * U * Hs), zero)
    grad = torch.stack([torch.where(va, gm, zero), gv], 1)
    bound = torch.stack([torch.where(va, b_gm, zero), b_gv], 1) + TINY
    return dict(loss=loss, bound_loss=bound_loss, count=n, grad=grad, bound_grad=bound, clamped=clamped)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all elements (0 / 0 counts as 0; a NaN error counts as inf); got may be fp32."""
    err = (got.detach().double().to(ref.device) - ref).abs()
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    r = torch.where(torch.isnan(err) | torch.isnan(r), torch.full_like(err, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).norm())


def torch_tail(depth, up_mask, gt_depth, gt_depth_mask):
    """The torch tail under autograd, in the dtype of its inputs: dnet.upsample_depth_via_mask + gaussian_activation(magnet=False) +
    the reference's loss expression (utils/losses.py:15-22).  depth (B,2,h,w), up_mask (B,144,h,w), gt_depth (B,1,4h,4w),
    gt_depth_mask (B,1,4h,4w) bool -> (loss, pred (B,2,4h,4w))."""
    from magnet_amd import dnet
    pred = dnet.gaussian_activation(dnet.upsample_depth_via_mask(depth, up_mask, 4), magnet=False)
    return reference_loss(pred, gt_depth, gt_depth_mask), pred


def reference_loss(pred, gt_depth, gt_depth_mask):
    """utils/losses.py:15-22."""
    gt = gt_depth[gt_depth_mask]
    mu, var = torch.split(pred, 1, dim=1)
    mu = mu[gt_depth_mask]
    var = var[gt_depth_mask]
    var[var < 1e-10] = 1e-10
    nll = (torch.square(mu - gt) / (2 * var)) + (0.5 * torch.log(var))
    return torch.mean(nll)


def emulate_fp32(depth, mask, gt, valid, grad_loss=1.0):
    """The kernels' arithmetic in numpy fp32, operation for operation (csrc/dnet_loss.hip): depth (B,2,h,w), mask (B,144,h,w), gt
    (B,4h,4w), valid (B,4h,4w) bool -> dict pred (B,2,4h,4w), loss, grad_depth, grad_mask.  The loss and the count are summed in
    float64 (numpy's own order: the kernel's fixed order differs by fp64 roundings only)."""
    f = np.float32
    depth = np.asarray(depth, f); gt = np.asarray(gt, f); valid = np.asarray(valid, bool)
    B, _, h, w = depth.shape
    L = np.asarray(mask, f).reshape(B, 9, 4, 4, h, w)
    pad = np.zeros((B, 2, h + 2, w + 2), f)
    pad[:, :, 1:-1, 1:-1] = depth
    o = [[pad[:, c, t // 3:t // 3 + h, t % 3:t % 3 + w].reshape(B, 1, 1, h, w) for t in range(9)] for c in range(2)]
    g = gt.reshape(B, h, 4, w, 4).transpose(0, 2, 4, 1, 3)
    va = valid.reshape(B, h, 4, w, 4).transpose(0, 2, 4, 1, 3)
    fine = lambda x: x.transpose(0, 3, 1, 4, 2).reshape(B, 4 * h, 4 * w)
    with np.errstate(all="ignore"):
        mx = np.full(L[:, 0].shape, -3.4e38, f)
        for t in range(9):
            mx = np.maximum(mx, L[:, t])
        e, den = [], np.zeros_like(mx)
        for t in range(9):
            e.append(np.exp(L[:, t] - mx))
            den = den + e[t]
        inv = f(1) / den
        wt = [e[t] * inv for t in range(9)]
        mu, vu = np.zeros_like(mx), np.zeros_like(mx)
        for t in range(9):
            mu = mu + wt[t] * o[0][t]
            vu = vu + wt[t] * o[1][t]
        var = (np.where(vu > 0, vu, np.expm1(vu)) + f(1)) + f(1e-10)
        assert all(x.dtype == f for x in (mu, vu, var, inv))
        cl = var < f(1e-10)
        vc = np.where(cl, f(1e-10), var)
        d = mu - g
        nll = d * d / (f(2) * vc) + f(0.5) * np.log(vc)
        n = int(va.sum())
        loss = f(nll[va].astype(np.float64).sum() / n) if n else f("nan")
        c = f(np.float64(f(grad_loss)) / n) if n else f(0)
        gm = np.where(va, c * (d / vc), f(0))
        de = np.where(vu > 0, f(1), np.exp(vu))
        gv = np.where(va & ~cl, c * (f(0.5) / vc - d * d / (f(2) * vc * vc)) * de, f(0))
        G = [gm * o[0][t] + gv * o[1][t] for t in range(9)]
        S = np.zeros_like(mx)
        for t in range(9):
            S = S + wt[t] * G[t]
        gmask = np.stack([wt[t] * (G[t] - S) for t in range(9)], 1).reshape(B, 144, h, w)
        part = np.zeros((B, 2, 9, h + 2, w + 2), f)                          # zero border: sources outside the image give nothing
        for ci, gc in enumerate((gm, gv)):
            for t in range(9):
                rows = []
                for i in range(4):                                           # j ascending inside a sub-row, then the sub-rows in order
                    acc = np.zeros((B, h, w), f)
                    for j in range(4):
                        acc = acc + wt[t][:, i, j] * gc[:, i, j]
                    rows.append(acc)
                part[:, ci, t, 1:-1, 1:-1] = ((rows[0] + rows[1]) + rows[2]) + rows[3]
        gd = np.zeros((B, 2, h, w), f)
        for t in range(9):
            dy, dx = t // 3 - 1, t % 3 - 1
            gd = gd + part[:, :, t, 1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
        assert gd.dtype == f and gmask.dtype == f and nll.dtype == f
    return dict(pred=np.stack([fine(mu), fine(var)], 1), loss=float(loss), grad_depth=gd, grad_mask=gmask)


def random_case(B, h, w, std, seed):
    """depth (B,2,h,w) [mu around 2.5, v around -1 +- 1.5: both branches of the ELU], logits of standard deviation std, gt (B,4h,4w),
    about half the pixels valid."""
    g = torch.Generator().manual_seed(seed)
    depth = torch.randn(B, 2, h, w, generator=g) * torch.tensor([1.0, 1.5]).view(1, 2, 1, 1) + torch.tensor([2.5, -1.0]).view(1, 2, 1, 1)
    mask = torch.randn(B, 144, h, w, generator=g) * std
    gt = torch.rand(B, 4 * h, 4 * w, generator=g) * 5.0 + 0.2
    valid = torch.rand(B, 4 * h, 4 * w, generator=g) < 0.5
    valid.view(-1)[0] = True
    return depth, mask, gt, valid


def pattern_case(pattern, depth, mask, gt):
    """Inputs that take the kernels' edge paths (CPU tensors)."""
    depth, mask, gt = depth.clone(), mask.clone(), gt.clone()
    B, _, h, w = depth.shape
    if pattern == "v_floor":                                                # var at its 1e-10 floor: elu(vu) + 1 is 0 in fp32
        depth[:, 1] = -20.5 - depth[:, 1].abs()
    elif pattern == "v_positive":
        depth[:, 1] = 0.1 + depth[:, 1].abs()
    elif pattern == "mu_equals_gt":                                         # d = 0 up to the rounding of nine equal weights: a constant mu away from the border
        mask.zero_()
        depth[:, 0] = 2.25
        gt.fill_(2.25)
    elif pattern == "one_tap_1e4":                                          # one tap at +1e4 (another one per sub-pixel), the rest at 0
        g = torch.Generator().manual_seed(3)
        m = torch.zeros(B, 9, 16, h, w)
        m.scatter_(1, torch.randint(0, 9, (B, 1, 16, h, w), generator=g), 1e4)
        mask = m.reshape(B, 144, h, w)
    elif pattern == "spread_88":                                            # overflows without the max subtraction
        m = mask.reshape(B, 9, 16, h, w) * 20.0
        m[:, 0], m[:, 8] = 44.0, -44.0
        mask = m.reshape(B, 144, h, w)
    elif pattern == "equal":
        mask = mask[:, :1].expand(B, 144, h, w).contiguous()
    else:
        raise ValueError(pattern)
    return depth, mask, gt


def plain_case(B=2, H=6, W=9):
    g = torch.Generator().manual_seed(11)
    pred = torch.stack([torch.randn(B, H, W, generator=g) + 2.5, torch.rand(B, H, W, generator=g) * 2 + 0.05], 1)
    gt = torch.rand(B, H, W, generator=g) * 5 + 0.2
    valid = torch.rand(B, H, W, generator=g) < 0.6
    special = [0.0, -1.0, 1e-12, 5e-11, 2e-10, 1e-9, -1e-30]                 # var <= 0 and var < 1e-10 are clamped, 2e-10 and 1e-9 are not
    pred[0, 1, 0, :len(special)] = torch.tensor(special)
    valid[0, 0, :len(special)] = True
    valid[0, 1, 0] = False; pred[0, 1, 1, 0] = 0.0                            # a clamped pixel outside the mask
    return pred, gt, valid, len(special)
