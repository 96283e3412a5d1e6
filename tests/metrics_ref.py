"""Float64 restatement of magnet_depth_metrics_ex (csrc/elementwise.hip) for the tests: the 13 per-frame sums for the three kinds of
second plane, the 12-entry metric row, and how far the kernel's sums may lie from the restated ones.

The reference form takes every pixel's term in numpy fp64 and adds the terms with math.fsum (the correctly rounded sum).  The kernel
computes the same terms in fp64 on the device and adds them in its own fixed order, so the two differ by

  * the rounding inside a term.  G and P are fp32 values, so d = G - P, d * d and sigma * sigma are exact in fp64 arithmetic up to one
    rounding; log, log10 and every division are taken as within one ulp (relative 2^-52 = EPS); the cancellations are carried as
    absolute errors: lg - lp is off by at most EPS (|lg| + |lp|), 1/G - 1/P by at most EPS (1/G + 1/P), and the products built on such
    a difference x with error e by 2 |x| e + e^2.  Every further operation adds EPS times its result.  The reference's own terms carry
    the same roundings (numpy's log is no better than the device's), so a term's bound counts twice;
  * the summation: adding n terms in any order is off by at most n 2^-53 sum|t| (first order, every partial sum is at most sum|t|);
    fsum adds at most half an ulp of the result, which the same expression covers with room.

Counts (sums 0, 9, 10, 11) are sums of ones, exact below 2^53 - provided every comparison falls the same way on both sides, which
`margins` establishes: the smallest relative distance of any pixel's t = max(G/P, P/G) to 1.25, 1.25^2, 1.25^3 and of any variance to
the 1e-6 clamp.  A distance above 1e-9 is seven orders above the two roundings (2^-52 each) that separate the two sides' t.
"""
import math

import numpy as np

EPS = 2.0 ** -52
LN_2PI = 1.8378770664093453
SIGMA, VARIANCE, NONE = 0, 1, 2
PARTS, THREADS = 64, 256                       # stage 1: workgroups per frame, threads per workgroup
ROW_ORDER = ("abs_rel", "abs_diff", "sq_rel", "rmse", "rmse_log", "irmse", "log_10", "silog", "a1", "a2", "a3", "nll")


def _pixels(mu, second, gt, kind, dmin, dmax, window):
    """One frame: flat index of the evaluated pixels and their G, P, variance-before-clamp (fp64 arrays; variance None under NONE).
    The masking and clamping are done in fp32, as the kernel does them."""
    gt = np.asarray(gt, dtype=np.float32)
    H, W = gt.shape
    dmin, dmax = np.float32(dmin), np.float32(dmax)
    g = gt.copy()
    g[g > dmax] = 0.0
    valid = np.logical_and(g > dmin, g < dmax)
    if window is not None:
        y0, y1, x0, x1 = window
        ev = np.zeros((H, W), dtype=bool)
        ev[y0:y1, x0:x1] = True
        valid &= ev
    p = np.asarray(mu, dtype=np.float32).copy()
    with np.errstate(invalid="ignore"):
        p = np.where(p < dmin, dmin, p)
        p = np.where(p > dmax, dmax, p)
    p = np.where(np.isnan(p), dmin, p)
    idx = np.flatnonzero(valid.reshape(-1))
    G = g.reshape(-1)[idx].astype(np.float64)
    P = p.reshape(-1)[idx].astype(np.float64)
    var = None
    if kind != NONE:
        s = np.asarray(second, dtype=np.float32).reshape(-1)[idx].astype(np.float64)
        var = s * s if kind == SIGMA else s
    return idx, G, P, var, H * W


def _terms(G, P, var, clamp=True):
    """The 13 per-pixel terms (13, n) and the bound of one side's rounding inside each of them (13, n)."""
    n = G.shape[0]
    T = np.zeros((13, n)); E = np.zeros((13, n))
    d = G - P
    lg, lp = np.log(G), np.log(P)
    t = np.maximum(G / P, P / G)
    T[0] = 1.0
    T[1] = np.abs(d)
    T[2] = np.abs(d) / G;                    E[2] = EPS * T[2]
    T[3] = d * d / G;                        E[3] = 2 * EPS * T[3]
    T[4] = d * d;                            E[4] = EPS * T[4]
    x = lg - lp; e = EPS * (np.abs(lg) + np.abs(lp)) + EPS * np.abs(x)
    T[5] = x * x;                            E[5] = 2 * np.abs(x) * e + e * e + EPS * T[5]
    T[6] = lp - lg;                          E[6] = e
    l10g, l10p = np.log10(G), np.log10(P)
    T[7] = np.abs(l10g - l10p);              E[7] = EPS * (np.abs(l10g) + np.abs(l10p)) + EPS * T[7]
    y = 1.0 / G - 1.0 / P; e = EPS * (1.0 / G + 1.0 / P) + EPS * np.abs(y)
    T[8] = y * y;                            E[8] = 2 * np.abs(y) * e + e * e + EPS * T[8]
    T[9], T[10], T[11] = t < 1.25, t < 1.25 * 1.25, t < 1.25 * 1.25 * 1.25
    if var is not None:
        v = np.where(var < 1e-6, 1e-6, var) if clamp else var
        lv, q = np.log(v), d * d / v
        T[12] = 0.5 * (lv + LN_2PI + q)
        E[12] = 0.5 * (EPS * np.abs(lv) + EPS * np.abs(lv + LN_2PI) + 2 * EPS * q + EPS * np.abs(lv + LN_2PI + q))
    return T, E, t


def frame_sums(mu, second, gt, kind, dmin, dmax, window=None):
    """One frame -> (sums[13] by math.fsum, bound[13]): |kernel sum - sums| <= bound."""
    _, G, P, var, _ = _pixels(mu, second, gt, kind, dmin, dmax, window)
    T, E, _ = _terms(G, P, var)
    n = G.shape[0]
    sums = np.array([math.fsum(T[k]) for k in range(13)])
    bound = np.array([2 * math.fsum(E[k]) + n * 2.0 ** -53 * math.fsum(np.abs(T[k])) for k in range(13)])
    bound[[0, 9, 10, 11]] = 0.0
    return sums, bound


def frame_sums_kernel_order(mu, second, gt, kind, dmin, dmax, window=None, clamp=True):
    """The same sums added as the kernel adds them: thread tid of workgroup blk takes the pixels blk * 256 + tid + k * 64 * 256 in
    turn, the 64 lanes of a wave are folded by the shuffle tree (offsets 32 ... 1, lane 0 holds the result), the 4 waves are added in
    order, and so are the 64 workgroups.  A pixel that is skipped adds nothing, as adding 0.0 does."""
    idx, G, P, var, HW = _pixels(mu, second, gt, kind, dmin, dmax, window)
    T, _, _ = _terms(G, P, var, clamp=clamp)
    stride = PARTS * THREADS
    passes = (HW + stride - 1) // stride
    full = np.zeros((13, passes * stride))
    full[:, idx] = T
    full = full.reshape(13, passes, PARTS, THREADS // 64, 64)
    acc = np.zeros((13, PARTS, THREADS // 64, 64))
    for k in range(passes):
        acc = acc + full[:, k]
    o = 32
    while o > 0:
        acc = acc[..., :o] + acc[..., o:2 * o]
        o >>= 1
    w = acc[..., 0]                                             # (13, PARTS, 4)
    part = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    out = np.zeros(13)
    for q in range(PARTS):
        out = out + part[:, q]
    return out


def margins(mu, second, gt, kind, dmin, dmax, window=None):
    """(smallest relative distance of any t to a threshold, smallest relative distance of any variance to 1e-6); inf without pixels
    or without a second plane."""
    _, G, P, var, _ = _pixels(mu, second, gt, kind, dmin, dmax, window)
    if G.shape[0] == 0:
        return math.inf, math.inf
    t = np.maximum(G / P, P / G)
    mt = min(float(np.min(np.abs(t - th) / th)) for th in (1.25, 1.25 * 1.25, 1.25 * 1.25 * 1.25))
    mv = math.inf if var is None else float(np.min(np.abs(var - 1e-6) / 1e-6))
    return mt, mv


def row_from_sums(s, kind):
    """One frame's sums -> its 12 metrics in ROW_ORDER, every operation a separately rounded fp64 one."""
    s = [np.float64(x) for x in s]
    n = s[0]
    if not n > 0:
        row = [np.float64("nan")] * 12
    else:
        mean_err = s[6] / n
        x = s[5] / n - mean_err * mean_err
        row = [s[2] / n, s[1] / n, s[3] / n, np.sqrt(s[4] / n), np.sqrt(s[5] / n), np.sqrt(s[8] / n), s[7] / n,
               np.sqrt(np.float64(0.0) if 0.0 > x else x) * np.float64(100.0), s[9] / n, s[10] / n, s[11] / n, s[12] / n]
    if kind == NONE:
        row[11] = np.float64(0.0)
    return [float(v) for v in row]


def make_case(B, H, W, kind, seed, dmin=1e-3, dmax=10.0):
    """Seeded inputs (mu, second or None, gt) as fp32 arrays (B, H, W): ground truth in (0.5, 9.5) with missing (0) and over-range
    pixels, predictions spread over all three thresholds with a few inf / nan / negative ones; sigma in [1e-4, 1.5) (so some
    sigma^2 fall under the clamp), variances 10 % in [1e-9, 1e-6), 10 % in (1, 4], the rest log-uniform in [1e-6, 1].  A single-pixel
    frame keeps its one pixel valid."""
    r = np.random.RandomState(seed)
    gt = (r.rand(B, H, W) * 9.0 + 0.5).astype(np.float32)
    mu = (gt * np.exp(r.randn(B, H, W) * 0.35)).astype(np.float32)
    if H * W > 4:
        u = r.rand(B, H, W)
        gt[u < 0.15] = 0.0
        gt[u > 0.95] = 12.0
        flat = mu.reshape(B, -1)
        flat[:, 1], flat[:, 2], flat[:, 3] = np.inf, np.nan, -1.0
    if kind == NONE:
        return mu, None, gt
    if kind == SIGMA:
        second = np.exp(r.rand(B, H, W) * (math.log(1.5) - math.log(1e-4)) + math.log(1e-4))
    else:
        u = r.rand(B, H, W)
        second = np.exp(r.rand(B, H, W) * (0.0 - math.log(1e-6)) + math.log(1e-6))
        lo = np.exp(r.rand(B, H, W) * (math.log(1e-6) - math.log(1e-9)) + math.log(1e-9)) * 0.999
        hi = 1.0 + r.rand(B, H, W) * 3.0 + 1e-3
        second = np.where(u < 0.1, lo, np.where(u > 0.9, hi, second))
    return mu, second.astype(np.float32), gt
