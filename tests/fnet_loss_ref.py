"""fp64 restatement of FnetLoss (magnet_amd/losses.py, csrc/fnet_loss.hip; the reference's inline loss, train_FNet.py:95-104) with
pointwise error bounds derived from the kernels' own arithmetic, the bin centres of the driver, and an fp32 emulation of the forward.

The restatement, per pixel over the D bins j:   m = max_j x_j,  a_j = m - x_j >= 0,  e_j = exp(-a_j),  Z = sum e_j,  p_j = e_j / Z,
pred = sum p_j d_j;  valid = gt > min_depth and not gt > max_depth;  loss = mean over valid of |pred - gt|;
grad_x_j = g p_j (d_j - pred) with g = grad_loss / count * sign(pred - gt) on valid pixels (sign(0) = 0) and 0 elsewhere.

Bounds.  u = 2^-24.  The forward kernel visits the bins in ascending order in chunks (CHUNK = 16 bins, then the D % 16 left over one
by one): per chunk, the running maximum moves to mn = max(m, chunk), Z and S are multiplied by sc = expf(m - mn), and every bin adds
e = expf(x_j - mn) to Z and fma(e, d_j, S) to S.  What the term of bin j carries into the final Z (and S) relative to e_j (e_j d_j):
  * the rounding of its exponent, (x_j - m_c)(1 + delta) with |delta| <= u, and of the exponent of every later rescale; the rescales
    telescope, m_c - x_j + sum (m_next - m_prev) = m - x_j = a_j, so all of them together cost a_j u: this is the term that grows with
    the spread of the logits, and it is damped by e_j itself (a e^-a <= 1 / e);
  * expf: within 2 ulp = 4 u relative (the device library documents 1 ulp);
  * each rescale after it: expf (4 u) and the product (u); there are at most R = D // 16 + D % 16 of them;
  * each addition after it: u (the fma rounds once); at most D.
So term j is off by at most (K + a_j) u with K = D + 5 R + 4, all terms of Z have one sign, those of S have one sign once weighted by
|d_j|, and with A = sum p_j |d_j|, Kz = sum p_j (K + a_j):
  |Z^ - Z| <= Kz u Z,    |S^ - S| <= u Z sum p_j |d_j| (K + a_j),    pred^ = fl(S^ / Z^):
  |pred^ - pred| <= 1.01 u [sum p_j |d_j| (K + a_j) + |pred| (Kz + 1)] + TINY (sum |d_j| + D |pred|)         (bound_pred)
(1.01: the second-order terms, K u < 3e-5 and a_j u e^(-a_j) small; TINY = 2^-126: an e_j below the normal range may lose all its
bits, or be flushed, and Z >= 1).  That is of the form c1(D) u sum p_j |d_j| with c1 = 2 (K + ln D) + 1 at most (sum p_j a_j <= ln D),
K = 109 at D = 80 and 340 at D = 256.  This is looser than a (2 D + small) u sketch at small D, where the bins left over after the last full
chunk go one by one and each is a rescale of its own (R = D % 16 for D < 16: c1 is about 47 at D = 3 and 227 at D = 80); the emulation
test prints the observed worst error over bound (about 0.04 - 0.07).
Loss: |pred^ - gt| is rounded once in fp32 (u), summed in fp64 over n valid pixels (n 2^-52) and the mean is stored in fp32 (u):
  |loss^ - loss| <= mean over valid of bound_pred + 1.01 u mean |pred - gt| + (u + n 2^-52) |loss|.          (bound_loss)
The count is exact (the same fp32 comparisons).
Backward: c = fl32(grad_loss / count) (u), t = fl(c rz) (u) with rz = fl(1 / Z^) (u + Kz u), e = expf(fl(x_j - m)) ((4 + a_j) u: m
is the exact maximum), fl(t e) (u), fl(d_j - pred^) (u, and pred^ itself is off by bound_pred), the last product (u):
  |grad^_j - grad_j| <= 1.01 |g| p_j [(Kz + a_j + 10) u |d_j - pred| + bound_pred] + TINY (1 + (1 + |g|) |d_j - pred|)   (bound_grad)
which is of the form c2(D) u |g| p_j (|d_j| + A).  Where |pred - gt| <= bound_pred + u |pred - gt| the kernel may see another sign
of pred^ - gt (or zero): such a pixel is marginal and its bound grows by 2 |g| p_j |d_j - pred|.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
CHUNK = 16                            # csrc/fnet_loss.hip: CH


def sid_centres(D: int, min_depth: float = 1e-3, max_depth: float = 10.0) -> torch.Tensor:
    """The driver's bin centres (train_FNet.py:56-65): spacing-increasing discretisation, centre of every bin, fp32 (D)."""
    idx = np.arange(D + 1)
    gamma = 1 - min_depth
    b = np.exp(np.log(max_depth + gamma) * idx / D) - gamma
    return torch.from_numpy(((b[:-1] + b[1:]) / 2).astype(np.float32))


def rescales(D: int, chunk: int = CHUNK) -> int:
    return D // chunk + D % chunk


def k_const(D: int, chunk: int = CHUNK) -> int:
    return D + 5 * rescales(D, chunk) + 4


def fnet_loss_ref(x, d, gt=None, min_depth=0.0, max_depth=0.0, grad_loss=1.0, chunk=CHUNK):
    """x (B,D,h,w), d (D), gt (B,h,w) or None: everything in float64 on x's device.  Returns a dict: pred, bound_pred; with gt also valid,
    count, loss, bound_loss, grad, bound_grad, marginal (number of marginal pixels)."""
    x = x.detach().double()
    B, D, h, w = x.shape
    dd = d.detach().double().reshape(1, D, 1, 1).to(x.device)
    m = x.amax(dim=1, keepdim=True)
    a = m - x
    e = torch.exp(-a)
    Z = e.sum(dim=1, keepdim=True)
    p = e / Z
    pred = (p * dd).sum(dim=1)
    K = k_const(D, chunk)
    pa = torch.where(p > 0, p * a, torch.zeros_like(p))                    # p = 0 where a is huge: the term is 0
    Kz = K + pa.sum(dim=1)
    wsum = (p * dd.abs()).sum(dim=1) * K + (pa * dd.abs()).sum(dim=1)
    bound_pred = 1.01 * U * (wsum + pred.abs() * (Kz + 1)) + TINY * (float(dd.abs().sum()) + D * pred.abs())
    out = dict(pred=pred, bound_pred=bound_pred)
    if gt is None:
        return out
    g32 = gt.detach().float().to(x.device)
    valid = (g32 > min_depth) & ~(g32 > max_depth)
    gt64 = g32.double()
    n = int(valid.sum())
    diff = pred - gt64
    if n:
        loss = float(diff.abs()[valid].sum() / n)
        bound_loss = float((bound_pred[valid].sum() + 1.01 * U * diff.abs()[valid].sum()) / n) + (U + n * 2.0 ** -52) * abs(loss)
    else:
        loss, bound_loss = float("nan"), 0.0
    g = torch.where(valid, torch.sign(diff), torch.zeros_like(diff)) * (float(grad_loss) / n if n else 0.0)
    dev = dd - pred.unsqueeze(1)
    grad = g.unsqueeze(1) * p * dev
    gabs = (torch.where(valid, torch.ones_like(diff), torch.zeros_like(diff)) * (abs(float(grad_loss)) / n if n else 0.0)).unsqueeze(1)
    bound_grad = 1.01 * gabs * p * ((Kz.unsqueeze(1) + a.clamp(max=1e30) + 10) * U * dev.abs() + bound_pred.unsqueeze(1)) \
        + TINY * (1 + (1 + gabs) * dev.abs())
    bound_grad = torch.where(p > 0, bound_grad, TINY * (1 + (1 + gabs) * dev.abs()))
    marginal = valid & (diff.abs() <= bound_pred + U * diff.abs())
    bound_grad = bound_grad + torch.where(marginal, torch.ones_like(diff), torch.zeros_like(diff)).unsqueeze(1) * 2 * gabs * p * dev.abs()
    out.update(valid=valid, count=n, loss=loss, bound_loss=bound_loss, grad=grad, bound_grad=bound_grad, marginal=int(marginal.sum()))
    return out


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all elements (0 / 0 counts as 0; a NaN error counts as inf); got may be fp32."""
    err = (got.detach().double().to(ref.device) - ref).abs()
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    r = torch.where(torch.isnan(err) | torch.isnan(r), torch.full_like(err, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def online_fp32(x: np.ndarray, d: np.ndarray, chunk: int = CHUNK):
    """The forward kernel's arithmetic in numpy fp32: x (B,D,h,w), d (D) -> (pred, m, rz), every operation rounded to fp32 (the fma of
    S in float64, rounded once: the product of two fp32 is exact there and the sum is rounded to fp32 from 53 bits)."""
    x = x.astype(np.float32); d = d.astype(np.float32)
    B, D, h, w = x.shape
    m = np.full((B, h, w), -np.inf, np.float32); Z = np.zeros((B, h, w), np.float32); S = np.zeros((B, h, w), np.float32)
    full = D - D % chunk
    groups = [(s, s + chunk) for s in range(0, full, chunk)] + [(j, j + 1) for j in range(full, D)]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for s, t in groups:
            mn = np.maximum(m, x[:, s:t].max(axis=1))
            sc = np.exp((m - mn).astype(np.float32)).astype(np.float32)
            Z = (Z * sc).astype(np.float32); S = (S * sc).astype(np.float32); m = mn
            for j in range(s, t):
                e = np.exp((x[:, j] - m).astype(np.float32)).astype(np.float32)
                Z = (Z + e).astype(np.float32)
                S = (e.astype(np.float64) * np.float64(d[j]) + S.astype(np.float64)).astype(np.float32)
    return (S / Z).astype(np.float32), m, (np.float32(1) / Z).astype(np.float32)


def driver_loss_torch(softmax_or_raw, d_center, gt_dmap, min_depth, max_depth, raw=True):
    """The driver's own expression (train_FNet.py:88, 96-104) in torch, in the dtype of its inputs, under autograd."""
    cv = torch.softmax(softmax_or_raw, dim=1) if raw else softmax_or_raw
    pred = torch.sum(cv * d_center.reshape(1, -1, 1, 1), dim=1, keepdim=True)
    gt = gt_dmap.clone()
    gt[gt > max_depth] = 0.0
    gt = torch.nn.functional.interpolate(gt, size=[pred.shape[2], pred.shape[3]], mode="nearest")
    mask = gt > min_depth
    return torch.mean(torch.abs(pred[mask] - gt[mask])), pred


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).norm())
