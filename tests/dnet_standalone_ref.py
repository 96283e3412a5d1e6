"""fp64 numpy restatement of magnet_dnet_upsample_gauss (csrc/dnet_kernels.hip) with the pointwise error bound of its fp32 arithmetic,
and the host restatement of test_DNet.py's validate() that eval_dnet.py is checked against.  Shared by tests/test_dnet_standalone_host.py
and tests/test_gpu_dnet_standalone.py.

The function (D_dense_depth.py:85-100 then DNET.py:55-60), for coarse pixel (y, x), sub-pixel (i, j), taps t = 0..8 at
(y + t // 3 - 1, x + t % 3 - 1):
    w[t]   = softmax_t mask[n, y, x, t*16 + i*4 + j]
    up[c]  = sum_t w[t] * head[n, c] at the tap, zero outside the image
    out    = [up[0], elu(up[1]) + 1 + 1e-10]                      at (n, :, 4y + i, 4x + j)
"""
import numpy as np

U = 2.0 ** -24                       # fp32 unit roundoff: one correctly rounded operation has relative error <= U
ULP1 = 2.0 * U                       # a 1-ulp library function (expf, expm1f of the device maths library) has relative error <= 2 U
FMIN = 2.0 ** -126                   # smallest normal fp32: an underflowing exp loses at most this much absolutely, denormals kept or flushed


def _grids(head, head_ld, mask, mask_ld, N, h, w):
    rows = N * (h + 2) * (w + 2)
    H = np.asarray(head, dtype=np.float64).reshape(-1, head_ld)[:rows].reshape(N, h + 2, w + 2, head_ld)[..., :2]
    Hp = np.zeros((N, h + 2, w + 2, 2))
    Hp[:, 1:-1, 1:-1] = H[:, 1:-1, 1:-1]                               # outside the image counts as zero, whatever the border rows hold
    M = np.asarray(mask, dtype=np.float64).reshape(-1, mask_ld)[:rows].reshape(N, h + 2, w + 2, mask_ld)
    return Hp, M[:, 1:-1, 1:-1, :144].reshape(N, h, w, 9, 4, 4)


def softmax_tap_terms(M, axis, d_err=1.0, exp_err=ULP1 / U):
    """The softmax over the 9 taps along `axis` of the logits M (fp64) as the kernels form it, and the rounding count of one tap's term:
    returns (d, wgt, K) with d = M - max (<= 0, the largest tap exactly 0), wgt = exp(d) / sum exp(d), and K[t] the number of roundings,
    in units of U, that the term w[t] * v[t] of the sum of 9 passes through (Higham's gamma_k, first order k U):
        d = x - max        1, an ABSOLUTE error U |d| in the exponent -> relative |d| U after exp           (d_err |d|)
        the exponential    2 = a 1-ulp expf                                                                (exp_err)
        the denominator    8 additions + the exp errors of its own terms, sum_m w[m] (d_err |d[m]| + exp_err)
        1 / den            1
        e * inv            1
        w * v              1
        the sum of 9       8 additions (the first one adds to zero and is exact)
    d_err and exp_err describe the exponential: the defaults are the device maths library's expf (dnet_upsample_gauss_kernel); the
    native exponential of upsample_kernel / upsample_cl_kernel passes its own (tests/elementwise_fwd_ref.py)."""
    d = M - M.max(axis=axis, keepdims=True)
    e = np.exp(d)
    wgt = e / e.sum(axis=axis, keepdims=True)
    a = d_err * np.abs(d) + exp_err
    K = a + 8.0 + (wgt * a).sum(axis=axis, keepdims=True) + 1.0 + 1.0 + 1.0 + 8.0
    return d, wgt, K


def convex_sum_bound(S, K, vmax):
    """S = sum_t w[t] |v[t]| K[t] -> the bound on the sum of 9: the first-order mass, Higham's 1 / (1 - k U) for the higher orders, plus
    9 taps whose exponential may have underflowed (each loses at most FMIN of weight, times the largest |v| of the neighbourhood)."""
    return S * U / (1.0 - float(K.max()) * U) + 9.0 * FMIN * vmax


def _elu1(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0))) + 1.0 + 1e-10


def upsample_gauss_ref(head, head_ld, mask, mask_ld, N, h, w, defect=None, with_bound=False):
    """fp64 restatement; returns out (N, 2, 4h, 4w) float64, and with_bound=True also the pointwise bound on |kernel - out|.
    defect: None, 'act_first' (activation at 1/4 resolution, then upsampling) or 'taps_transposed' (tap t read at (t % 3, t // 3))."""
    Hp, M = _grids(head, head_ld, mask, mask_ld, N, h, w)
    if defect == "act_first":
        Hp = Hp.copy()
        Hp[:, 1:-1, 1:-1, 1] = _elu1(Hp[:, 1:-1, 1:-1, 1])
    d, wgt, K = softmax_tap_terms(M, axis=3)                            # wgt (N, h, w, 9, 4, 4)
    up = np.zeros((N, 2, h, w, 4, 4))
    S = np.zeros((N, 2, h, w, 4, 4))                                    # sum_t w[t] |v[t]| K[t], the first-order error mass
    vmax = np.zeros((N, 2, h, w, 1, 1))
    for t in range(9):
        ty, tx = (t % 3, t // 3) if defect == "taps_transposed" else (t // 3, t % 3)
        v = Hp[:, ty:ty + h, tx:tx + w, :].transpose(0, 3, 1, 2)[..., None, None]           # (N, 2, h, w, 1, 1)
        up += wgt[:, None, :, :, t] * v
        S += wgt[:, None, :, :, t] * np.abs(v) * K[:, None, :, :, t]
        vmax = np.maximum(vmax, np.abs(v))
    if defect != "act_first":
        s = up[:, 1].copy()
        up[:, 1] = _elu1(s)
    out = up.transpose(0, 1, 2, 4, 3, 5).reshape(N, 2, 4 * h, 4 * w)
    if not with_bound:
        return out
    E = convex_sum_bound(S, K, vmax)
    Eb = np.empty_like(E)
    Eb[:, 0] = E[:, 0]
    # variance: elu is 1-Lipschitz, so the error of its argument passes through at most unchanged (across the knee too); expm1f is 1 ulp
    # of |elu(s)| <= max(1, s); "+ 1" and "+ 1e-10" are one rounding each of a value <= the result; 1e-10 itself is rounded to fp32 once
    elu = np.abs(up[:, 1] - 1.0 - 1e-10)
    Eb[:, 1] = (E[:, 1] + ULP1 * elu + 2.0 * U * np.abs(up[:, 1]) + 1e-10 * U) * (1.0 + 4.0 * U)
    return out, Eb.transpose(0, 1, 2, 4, 3, 5).reshape(N, 2, 4 * h, 4 * w)


def pad_cl(x_nchw, ld, fill=0.0):
    """(N, C, h, w) -> the convolution kernel's padded channel-last rows (N*(h+2)*(w+2), ld), channels [0, C); everything else `fill`."""
    x = np.asarray(x_nchw)
    N, C, h, w = x.shape
    out = np.full((N, h + 2, w + 2, ld), fill, dtype=x.dtype)
    out[:, 1:-1, 1:-1, :C] = x.transpose(0, 2, 3, 1)
    return out.reshape(-1, ld)


def validate_host(outs, gts, min_depth, max_depth, crop=None):
    """test_DNet.py:40-71 + utils.compute_depth_errors (utils/utils.py:106-144) + RunningAverageDict in float64 numpy: outs = list of
    (1, 2, H, W) [mu, variance] model outputs, gts = list of (1, 1, H, W)."""
    tot, n = None, 0
    for out, gt in zip(outs, gts):
        gt = np.asarray(gt, dtype=np.float64)[0, 0]
        pred = np.asarray(out, dtype=np.float64)[0, 0].copy()
        var = np.asarray(out, dtype=np.float64)[0, 1].copy()
        valid = np.logical_and(gt > min_depth, gt < max_depth)
        if crop is not None:
            H, W = gt.shape
            ev = np.zeros(valid.shape, dtype=bool)
            if crop == "garg":
                ev[int(0.40810811 * H):int(0.99189189 * H), int(0.03594771 * W):int(0.96405229 * W)] = True
            else:
                ev[int(0.3324324 * H):int(0.91351351 * H), int(0.0359477 * W):int(0.96405229 * W)] = True
            valid = np.logical_and(valid, ev)
        pred[pred < min_depth] = min_depth
        pred[pred > max_depth] = max_depth
        pred[np.isinf(pred)] = max_depth
        pred[np.isnan(pred)] = min_depth
        g, p, v = gt[valid], pred[valid], var[valid]
        thresh = np.maximum(g / p, p / g)
        err = np.log(p) - np.log(g)
        v[v < 1e-6] = 1e-6
        m = dict(a1=(thresh < 1.25).mean(), a2=(thresh < 1.25 ** 2).mean(), a3=(thresh < 1.25 ** 3).mean(),
                 abs_diff=np.mean(np.abs(g - p)), abs_rel=np.mean(np.abs(g - p) / g), sq_rel=np.mean((g - p) ** 2 / g),
                 rmse=np.sqrt(((g - p) ** 2).mean()), log_10=np.abs(np.log10(g) - np.log10(p)).mean(),
                 irmse=np.sqrt(((1 / g - 1 / p) ** 2).mean()), rmse_log=np.sqrt((err ** 2).mean()),
                 silog=np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100,
                 nll=np.mean(0.5 * (np.log(v) + np.log(2 * np.pi) + np.square(g - p) / v)))
        tot = m if tot is None else {k: (m[k] + n * tot[k]) / (n + 1) for k in m}
        n += 1
    return {k: float(v) for k, v in tot.items()}
