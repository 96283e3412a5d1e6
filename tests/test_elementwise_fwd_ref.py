"""CPU: (a) the fp64 restatements of tests/elementwise_fwd_ref.py equal the textbook float64 forms (F.elu, the reference model's
F.unfold(padding=1) + softmax over the 9 taps, F.conv2d(stride=2, padding=1), F.avg_pool2d, F.interpolate(align_corners=True)) to
1e-12; (b) an fp32 emulation of each kernel's arithmetic in the kernel's order stays inside the derived bound on the very inputs the
GPU tests use (tests/test_gpu_elementwise_fwd.py; cases, seeds and generators come from the module); (c) each planted defect of that
emulation exceeds the bound somewhere on those inputs.

The bilinear restatement forms its weights in the kernel's fp32 coordinate arithmetic, so it cannot equal a float64 interpolation to
1e-12 where the scale is not an fp32 number; (a) therefore checks the SAME gather with coords="exact" (float64 coordinates) against
F.interpolate to 1e-12, and the kernel-coordinate form against the exact one within the rounding of the coordinates themselves."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from magnet_amd.planes import split_bf16, to_f16_sat
from tests import elementwise_fwd_ref as R

f32 = np.float32


def _ratio(got, ref, bound):
    return R.ratio(torch.as_tensor(got), ref, bound)[0]


def _store(v32, fmt):
    """The value the kernel's store leaves, read back as the tests read it (float64)."""
    if fmt == "f16":
        return to_f16_sat(v32).double()
    hi, lo = split_bf16(v32)
    return hi.double() + lo.double()


# ---- fp32 emulations, with the planted defects ------------------------------------------------------------------------------------------
def emu_gaussian(o, g, defect=None):
    o, g = torch.as_tensor(o), torch.as_tensor(g)
    mu0, sg0, o0, o1 = g[:, 0], g[:, 1], o[:, 0], o[:, 1]
    e = torch.where(o1 > 0, o1, torch.expm1(o1.double().clamp_max(0.0)).float())          # a correctly rounded expm1f
    sg1 = ((e + 1.0) + torch.tensor(1e-10, dtype=torch.float32)) * sg0
    mu1 = mu0 + o0 * (sg1 if defect == "mu_from_sg1" else sg0)
    return torch.stack([mu1, sg1], 1)


def emu_gauss_head(x):
    x = torch.as_tensor(x)
    o1 = x[:, 1]
    e = torch.where(o1 > 0, o1, torch.expm1(o1.double().clamp_max(0.0)).float())
    return torch.stack([x[:, 0], ((e + 1.0) + torch.tensor(1e-10, dtype=torch.float32)).sqrt()], 1)


def emu_upsample(depth, logits, defect=None):
    """upsample_kernel<K, C> / upsample_cl_kernel in numpy fp32: depth (P, B, C, h, w), logits (B, 9, K, K, h, w)."""
    D, L = np.asarray(depth, dtype=f32), np.asarray(logits, dtype=f32)
    P, B, C, h, w = D.shape
    K = L.shape[2]
    if defect == "subpixel_transposed":
        L = L.transpose(0, 1, 3, 2, 4, 5)                                                 # channel j K + i
    d = L - L.max(axis=1, keepdims=True)
    p = f32(R.LOG2E_F32) * d
    e = np.exp2(p.astype(np.float64)).astype(f32)                                         # a correctly rounded exp2, inside E_NATIVE
    e[e < f32(2.0 ** -126)] = 0                                                           # the instruction flushes denormal results
    den = np.zeros_like(e[:, 0])
    for t in range(9):
        den = den + e[:, t]
    wg = e if defect == "not_normalised" else e * (f32(1.0) / den)[:, None]
    Dp = np.pad(D, ((0, 0), (0, 0), (0, 0), (1, 1), (1, 1)), mode="edge" if defect == "border_clamped" else "constant")
    if defect == "channel1_from_channel0":
        Dn = Dp[:, :, [0] * C]                                                            # every channel convolved from channel 0's neighbourhood
    else:
        Dn = Dp
    a = np.zeros((P, B, C, K, K, h, w), dtype=f32)
    for t in range(9):
        ty, tx = (t % 3, t // 3) if defect == "taps_transposed" else (t // 3, t % 3)
        v = Dn[..., ty:ty + h, tx:tx + w][:, :, :, None, None]
        a = a + wg[None, :, None, t] * v
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 1, 2, 5, 3, 6, 4)).reshape(P, B, C, h * K, w * K))


def emu_stem(img, wgt, bias, fmt, defect=None):
    N, _, H, W = img.shape
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros((N, 3, 2 * H2 + 2, 2 * W2 + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = img
    s = 1 if defect == "taps_unshifted" else 0                                            # reads 2y + dy instead of 2y + dy - 1
    acc = torch.zeros((N, H2, W2, 32))
    for ci in range(3):
        for dy in range(3):
            for dx in range(3):
                tap = xp[:, ci, dy + s:dy + s + 2 * H2:2, dx + s:dx + s + 2 * W2:2][..., None]
                acc = (wgt[:, ci * 9 + dy * 3 + dx].double() * tap.double() + acc.double()).float()       # fmaf
    return _store((acc + bias).clamp_min(0.0), fmt)


def emu_avgpool(buf32, C, k, fmt, defect=None):
    """buf32: the fp32 values of the whole buffer as the kernel's load forms them (fp16 -> fp32, or hi + lo in fp32)."""
    N, h, w, pad, ld, c0 = R.AVGPOOL_GRID
    ph, pw = h // k, w // k
    o = 0 if defect == "window_without_pad" else pad
    win = buf32[:, o:o + ph * k, o:o + pw * k, c0:c0 + C].reshape(N, ph, k, pw, k, C).permute(0, 1, 3, 2, 4, 5).reshape(N * ph * pw, k * k, C)
    part = [torch.zeros((N * ph * pw, C)) for _ in range(16)]
    for e in range(k * k):
        part[e % 16] = part[e % 16] + win[:, e]
    s = torch.zeros((N * ph * pw, C))
    for sl in range(16):
        s = s + part[sl]
    return _store(s * (torch.tensor(1.0) / torch.tensor(float(k * k))), fmt)


def emu_bilinear(q_rows, ph, pw, h, w, fmt, defect=None):
    """q_rows: the flat (rows, C) fp32 input INCLUDING the rows behind the last image (an index past the grid reads them)."""
    N = R.BILINEAR_N

    def axis(n_in, n_out, clamp=True):
        if defect == "half_pixel":
            f = ((torch.arange(n_out, dtype=torch.float32) + 0.5) * (torch.tensor(float(n_in)) / torch.tensor(float(n_out))) - 0.5).clamp_min(0.0)
        else:
            s = (torch.tensor(float(n_in - 1)) / torch.tensor(float(n_out - 1))) if n_out > 1 else torch.tensor(0.0)
            f = s * torch.arange(n_out, dtype=torch.float32)
        i0 = f.to(torch.int64)
        i1 = i0 + ((i0 < n_in - 1).to(torch.int64) if clamp else 1)
        l1 = f - i0.float()
        return i0, i1, 1.0 - l1, l1
    y0, y1, ly0, ly1 = axis(ph, h, clamp=defect != "y1_unclamped")
    x0, x1, lx0, lx1 = axis(pw, w)
    n = torch.arange(N)[:, None, None] * (ph * pw)

    def at(yy, xx):
        return q_rows[n + yy[None, :, None] * pw + xx[None, None, :]]                      # (N, h, w, C)
    lx0, lx1, ly0, ly1 = lx0[None, None, :, None], lx1[None, None, :, None], ly0[None, :, None, None], ly1[None, :, None, None]
    v = ly0 * (lx0 * at(y0, x0) + lx1 * at(y0, x1)) + ly1 * (lx0 * at(y1, x0) + lx1 * at(y1, x1))
    return _store(v, fmt)


def emu_space_to_depth(x, defect=None):
    N, H2, W2, C = x.shape
    H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
    xs = torch.zeros((N, 2 * H4, 2 * W4, C), dtype=x.dtype)
    xs[:, :H2, :W2] = x
    if defect == "phases_swapped":
        return torch.cat([xs[:, py::2, px::2] for px in (0, 1) for py in (0, 1)], dim=3)
    return torch.cat([xs[:, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=3)


def _buf32(buf, fmt):
    if fmt == "f16":
        return to_f16_sat(buf).float()
    hi, lo = split_bf16(buf)
    return hi.float() + lo.float()


# ---- (a) the restatements against the textbook float64 forms --------------------------------------------------------------------------
def test_gaussian_update_ref_is_the_elu_formula():
    o, g = (torch.from_numpy(a).double() for a in R.gaussian_inputs(3, 7, 37))
    ref, bound = R.gaussian_update_ref(o, g)
    exp = torch.stack([g[:, 0] + o[:, 0] * g[:, 1], (F.elu(o[:, 1]) + 1.0 + 1e-10) * g[:, 1]], 1)
    torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)
    assert (bound > 0).all()
    # where elu + 1 cancels the bound is absolute, about 2 u sg0: far above the 1e-10 sg0 that an fp64 bound therefore cannot see
    low = o[:, 1] <= -20
    assert low.any() and (bound[:, 1][low] >= 1.9 * R.U * g[:, 1][low]).all() and (bound[:, 1][low] > 100 * 1e-10 * g[:, 1][low]).all()


def test_gauss_head_ref_is_the_elu_formula():
    x = torch.from_numpy(R.gauss_head_inputs(3, 7, 11)).double()
    ref, bound = R.gauss_head_ref(x)
    torch.testing.assert_close(ref[:, 1], (F.elu(x[:, 1]) + 1.0 + 1e-10).sqrt(), rtol=1e-12, atol=1e-12)
    assert torch.equal(ref[:, 0], x[:, 0]) and not bound[:, 0].any() and (bound[:, 1] > 0).all()


@pytest.mark.parametrize("K,C", R.UPSAMPLE_KC)
def test_convex_upsample_ref_is_unfold_softmax(K, C):
    B, h, w = 2, 6, 7
    depth, logits = R.upsample_inputs(B, h, w, K, C)
    ref, bound = R.convex_upsample_ref(depth, R.logits_nchw(logits, K))
    d, m = torch.from_numpy(depth[0]).double(), torch.from_numpy(logits).double()
    m = torch.softmax(m.view(B, 1, 9, K, K, h, w), dim=2)
    nb = F.unfold(d, [3, 3], padding=1).view(B, C, 9, 1, 1, h, w)
    exp = (m * nb).sum(dim=2).permute(0, 1, 4, 2, 5, 3).reshape(B, C, K * h, K * w)
    torch.testing.assert_close(ref[0], exp, rtol=1e-12, atol=1e-12)
    assert (bound > 0).all() and bound.shape == ref.shape


def test_logits_cl_is_the_nchw_view():
    B, h, w, ld = 2, 5, 7, 160
    _, pad, logits = R.upsample_cl_inputs(B, h, w, ld, 1)
    assert np.array_equal(R.logits_cl(pad, ld, B, h, w), R.logits_nchw(logits, 4))


@pytest.mark.parametrize("N,H,W", R.STEM_SHAPES)
def test_stem_ref_is_conv2d_stride2(N, H, W):
    img, wgt, b = R.stem_inputs(N, H, W)
    ref, _ = R.stem_ref(img, wgt, b, "planes")
    exp = F.relu(F.conv2d(img.double(), wgt.double().reshape(32, 3, 3, 3), b.double(), stride=2, padding=1)).permute(0, 2, 3, 1)
    torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k", [8, 16])
def test_avgpool_ref_is_avg_pool2d(k):
    N, h, w, pad, ld, c0 = R.AVGPOOL_GRID
    x = R.avgpool_inputs()[:, pad:-pad, pad:-pad, c0:c0 + 64].double()
    ref, _ = R.avgpool_ref(x, k, "f16")
    exp = F.avg_pool2d(x.permute(0, 3, 1, 2), k, k).permute(0, 2, 3, 1).reshape(-1, 64)
    torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("ph,pw,h,w", sorted({c[:4] for c in R.BILINEAR_CASES}))
def test_bilinear_ref_is_interpolate_align_corners(ph, pw, h, w):
    q = R.bilinear_inputs(ph, pw)[:R.BILINEAR_N * ph * pw].reshape(R.BILINEAR_N, ph, pw, -1)
    exact, _ = R.bilinear_ref(q, h, w, "planes", coords="exact")
    exp = F.interpolate(q.double().permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    torch.testing.assert_close(exact, exp, rtol=1e-12, atol=1e-12)
    # the kernel's fp32 coordinates: scale, product and the subtraction are one rounding each of numbers below max(ph, pw), per axis
    ref, _ = R.bilinear_ref(q, h, w, "planes")
    assert float((ref - exact).abs().max()) <= 2 * 3 * R.U * max(ph, pw) * 2 * float(q[:R.BILINEAR_N * ph * pw].abs().max())


def test_moves_are_moves():
    x = torch.arange(2 * 5 * 3 * 8, dtype=torch.float32).reshape(2, 5, 3, 8)
    out = R.space_to_depth_ref(x)
    assert out.shape == (2, 3, 2, 32)
    for y in range(3):
        for xx in range(2):
            for py in (0, 1):
                for px in (0, 1):
                    exp = x[:, 2 * y + py, 2 * xx + px] if 2 * y + py < 5 and 2 * xx + px < 3 else torch.zeros(2, 8)
                    assert torch.equal(out[:, y, xx, (py * 2 + px) * 8:(py * 2 + px + 1) * 8], exp)
    g = R.pack_gmm_inputs(3, 13, 21)
    p = R.pack_gmm_ref(g)
    assert torch.equal(p[:, 1:-1, 1:-1, 0], g[:, 0]) and torch.equal(p[:, 1:-1, 1:-1, 1], g[:, 1])
    assert not p[:, 0].any() and not p[:, -1].any() and not p[:, :, 0].any() and not p[:, :, -1].any()


# ---- (b) the emulations inside the bounds, (c) the planted defects outside them, on the GPU tests' inputs ------------------------------
@pytest.mark.parametrize("B,h,w", R.GAUSS_SHAPES)
def test_gaussian_update_emulation_and_defect(B, h, w):
    o, g = R.gaussian_inputs(B, h, w)
    ref, bound = R.gaussian_update_ref(o, g)
    assert _ratio(emu_gaussian(o, g), ref, bound) <= 1.0
    assert _ratio(emu_gaussian(o, g, "mu_from_sg1"), ref, bound) > 1.0


@pytest.mark.parametrize("N,h,w,pad,in_ld", R.GAUSS_HEAD_CASES)
def test_gauss_head_emulation(N, h, w, pad, in_ld):
    x = R.gauss_head_inputs(N, h, w)
    ref, bound = R.gauss_head_ref(x)
    assert _ratio(emu_gauss_head(x), ref, bound) <= 1.0


UPSAMPLE_DEFECTS = ["taps_transposed", "subpixel_transposed", "border_clamped", "not_normalised", "channel1_from_channel0"]


def _visible(defect, K, C, h, w):
    """Where a defect changes the function at all: a 1 x 1 image has one tap inside, K = 1 one sub-pixel, C = 1 one channel."""
    if defect == "subpixel_transposed":
        return K > 1
    if defect == "channel1_from_channel0":
        return C > 1
    if defect == "taps_transposed":
        return h > 1 and w > 1
    return True


@pytest.mark.parametrize("B,h,w", R.UPSAMPLE_SHAPES)
@pytest.mark.parametrize("K,C", R.UPSAMPLE_KC)
def test_upsample_emulation_and_defects(K, C, B, h, w):
    depth, logits = R.upsample_inputs(B, h, w, K, C)
    L = R.logits_nchw(logits, K)
    ref, bound = R.convex_upsample_ref(depth, L)
    assert _ratio(emu_upsample(depth, L), ref, bound) <= 1.0
    for defect in UPSAMPLE_DEFECTS:
        if _visible(defect, K, C, h, w):
            assert _ratio(emu_upsample(depth, L, defect), ref, bound) > 1.0, defect


@pytest.mark.parametrize("B,h,w,ld,n_pred", R.UPSAMPLE_CL_CASES)
def test_upsample_cl_emulation_and_defects(B, h, w, ld, n_pred):
    depth, mask_pad, _ = R.upsample_cl_inputs(B, h, w, ld, n_pred)
    L = R.logits_cl(mask_pad, ld, B, h, w)
    ref, bound = R.convex_upsample_ref(depth, L)
    assert _ratio(emu_upsample(depth, L), ref, bound) <= 1.0
    for defect in UPSAMPLE_DEFECTS:
        if _visible(defect, 4, 2, h, w):
            assert _ratio(emu_upsample(depth, L, defect), ref, bound) > 1.0, defect
    # a kernel that read a border row or a spare channel of the padded mask would see MASK_FILL win the softmax
    full = np.asarray(mask_pad).reshape(B, h + 2, w + 2, ld)
    shifted = full[:, :-2, :-2, :144].reshape(B, h, w, 9, 4, 4).transpose(0, 3, 4, 5, 1, 2)          # the grid read without its border offset
    assert _ratio(emu_upsample(depth, shifted), ref, bound) > 1.0


@pytest.mark.parametrize("fmt", ["planes", "f16"])
@pytest.mark.parametrize("N,H,W", R.STEM_SHAPES)
def test_stem_emulation_and_defect(N, H, W, fmt):
    img, wgt, b = R.stem_inputs(N, H, W)
    ref, bound = R.stem_ref(img, wgt, b, fmt)
    assert _ratio(emu_stem(img, wgt, b, fmt), ref, bound) <= 1.0
    assert _ratio(emu_stem(img, wgt, b, fmt, "taps_unshifted"), ref, bound) > 1.0


@pytest.mark.parametrize("fmt", ["planes", "f16"])
@pytest.mark.parametrize("C,k", R.AVGPOOL_CASES)
def test_avgpool_emulation_and_defect(C, k, fmt):
    N, h, w, pad, ld, c0 = R.AVGPOOL_GRID
    b32 = _buf32(R.avgpool_inputs(), fmt)
    held = _store(R.avgpool_inputs(), fmt)                                                # what the planes hold, in float64
    ref, bound = R.avgpool_ref(held[:, pad:-pad, pad:-pad, c0:c0 + C], k, fmt)
    assert _ratio(emu_avgpool(b32, C, k, fmt), ref, bound) <= 1.0
    assert _ratio(emu_avgpool(b32, C, k, fmt, "window_without_pad"), ref, bound) > 1.0


@pytest.mark.parametrize("fmt", ["planes", "f16"])
@pytest.mark.parametrize("ph,pw,h,w", sorted({c[:4] for c in R.BILINEAR_CASES}))
def test_bilinear_emulation_and_defects(ph, pw, h, w, fmt):
    rows = R.bilinear_inputs(ph, pw)
    q = rows[:R.BILINEAR_N * ph * pw].reshape(R.BILINEAR_N, ph, pw, -1)
    ref, bound = R.bilinear_ref(q, h, w, fmt)
    assert _ratio(emu_bilinear(rows, ph, pw, h, w, fmt), ref, bound) <= 1.0
    # y1 = y0 + 1 past the last row reads the rows behind the image: NaN behind the last one, whatever weight it gets
    assert _ratio(emu_bilinear(rows, ph, pw, h, w, fmt, "y1_unclamped"), ref, bound) > 1.0
    if (ph, pw) != (1, 1) and (ph, pw) != (h, w):                                         # one input texel, or scale 1: both rules are the same function
        assert _ratio(emu_bilinear(rows, ph, pw, h, w, fmt, "half_pixel"), ref, bound) > 1.0


@pytest.mark.parametrize("H2,W2", sorted({c[:2] for c in R.S2D_CASES}))
def test_space_to_depth_emulation_and_defect(H2, W2):
    x, _ = R.s2d_inputs(H2, W2)
    ref = R.space_to_depth_ref(x)
    assert torch.equal(emu_space_to_depth(x), ref)
    if (H2, W2) != (1, 1):                                                                # one texel: phases (0,1) and (1,0) are both beyond the edge
        assert not torch.equal(emu_space_to_depth(x, "phases_swapped"), ref)
