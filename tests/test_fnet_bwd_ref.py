"""CPU: the fp64 restatements of tests/fnet_bwd_ref.py equal torch float64 autograd of the PSMNet operations they restate, at odd
shapes, and each checker rejects a planted defect that a 2e-2 relative-L2 bar on the whole tensor accepts."""
import pytest
import torch
import torch.nn.functional as F

from magnet_amd.convnet import split_bf16
from magnet_amd.train_fnet import dgrad_pack, dgrad_pack_s2d, s2d_grad_to_3x3
from tests import fnet_bwd_ref as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _grid(x_nchw, pad):
    """(N, C, h, w) -> the zero-bordered channel-last rows (N*(h+2pad)*(w+2pad), C)."""
    N, C, h, w = x_nchw.shape
    out = torch.zeros((N, h + 2 * pad, w + 2 * pad, C), dtype=x_nchw.dtype)
    out[:, pad:pad + h, pad:pad + w] = x_nchw.permute(0, 2, 3, 1)
    return out.reshape(-1, C)


def _interior(rows, N, h, w, pad):
    return rows.reshape(N, h + 2 * pad, w + 2 * pad, -1)[:, pad:pad + h, pad:pad + w].permute(0, 3, 1, 2)


# ---- the restatements against autograd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
def test_bn_backward_ref_is_batchnorm_autograd(relu):
    N, C, h, w, pad = 3, 16, 5, 7, 2
    x = (torch.randn(N, C, h, w, generator=_g(1), dtype=torch.float64) * 2 + 1).requires_grad_()
    bn = torch.nn.BatchNorm2d(C).double().train()
    bn.weight.data.normal_(generator=_g(2)); bn.bias.data.normal_(generator=_g(3))
    y = bn(x)
    if relu:
        y = torch.relu(y)
    gy = torch.randn(y.shape, generator=_g(4), dtype=torch.float64)
    y.backward(gy)
    mean = x.detach().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(x.detach().var((0, 2, 3), unbiased=False) + bn.eps)
    r = R.bn_backward_ref(_grid(x.detach(), pad), (N, h + 2 * pad, w + 2 * pad, pad, C), mean, invstd, bn.weight.detach(),
                          bn.bias.detach(), relu, _grid(gy, pad))
    assert r["marginal"] == 0
    torch.testing.assert_close(_interior(r["dx"][0], N, h, w, pad), x.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(r["dgamma"][0], bn.weight.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(r["dbeta"][0], bn.bias.grad, rtol=1e-10, atol=1e-12)
    assert not r["dx"][0].reshape(N, h + 2 * pad, w + 2 * pad, C)[:, :pad].any()


@pytest.mark.parametrize("h,w,k", [(67, 131, 64), (67, 131, 8), (120, 160, 32), (64, 64, 16)])
def test_spp_refs_are_pool_and_upsample_autograd(h, w, k):
    N, pad = 2, 2
    ph, pw = h // k, w // k
    q = torch.randn(N, 32, ph, pw, generator=_g(5), dtype=torch.float64, requires_grad=True)
    gy = torch.randn(N, 32, h, w, generator=_g(6), dtype=torch.float64)
    F.interpolate(q, size=(h, w), mode="bilinear", align_corners=True).backward(gy)
    g = torch.zeros(N * (h + 2 * pad) * (w + 2 * pad), 320, dtype=torch.float64)
    g[:, 288:320] = _grid(gy, pad)
    ref, bound = R.spp_upsample_bwd_ref(g, 288, N, h, w, pad, ph, pw)
    torch.testing.assert_close(ref, q.grad.permute(0, 2, 3, 1).reshape(-1, 32), rtol=1e-11, atol=1e-12)
    assert (bound > 0).all()
    # the pool backward: the concat slice plus AvgPool2d(k, k) (floor mode) of the four branches
    x = torch.zeros(N, 128, h, w, dtype=torch.float64, requires_grad=True)
    dpools, loss = [], 0
    for kk in (64, 32, 16, 8):
        d = torch.randn(N, 128, h // kk, w // kk, generator=_g(kk), dtype=torch.float64)
        dpools.append(d.permute(0, 2, 3, 1).reshape(-1, 128))
        loss = loss + (F.avg_pool2d(x, kk, kk) * d).sum()
    loss.backward()
    gs = torch.randn(N * (h + 2 * pad) * (w + 2 * pad), 320, generator=_g(7), dtype=torch.float64)
    ref, bound = R.spp_pool_bwd_ref(gs, 64, N, h, w, pad, dpools)
    exp = x.grad.permute(0, 2, 3, 1) + gs.reshape(N, h + 2 * pad, w + 2 * pad, 320)[:, pad:pad + h, pad:pad + w, 64:192]
    torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)
    band = torch.zeros(N, h, w, 1, dtype=torch.bool)
    band[:, (h // 8) * 8:] = True
    band[:, :, (w // 8) * 8:] = True
    assert bool(band.any()) == (h % 8 != 0 or w % 8 != 0)
    assert not (bound * band).any()                                         # the remainder band: bit-exact


@pytest.mark.parametrize("dil", [1, 2])
def test_conv_ref_is_dilated_conv_and_its_input_gradient(dil):
    """conv_ref over a bordered grid == conv2d (dilation 1, 2); over the flipped transposed pack == conv2d_input."""
    N, cin, cout, h, w, pad = 2, 8, 16, 7, 9, 2
    x = torch.randn(N, cin, h, w, generator=_g(8), dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=_g(9)).to(torch.bfloat16).double()   # bf16-exact: the pack's lo is zero
    hi, lo = split_bf16(wt.float().permute(2, 3, 0, 1).reshape(9, cout, cin).contiguous())
    ref, _ = R.conv_ref(_grid(x, pad), R.join(hi, lo), 9, w + 2 * pad, N * (h + 2 * pad) * (w + 2 * pad), dil=dil)
    torch.testing.assert_close(_interior(ref, N, h, w, pad), F.conv2d(x, wt, padding=dil, dilation=dil), rtol=1e-12, atol=1e-12)
    dz = torch.randn(N, cout, h, w, generator=_g(10), dtype=torch.float64)
    dh, dl = dgrad_pack(wt.float())
    add = torch.randn(N * (h + 2 * pad) * (w + 2 * pad), cin, generator=_g(11), dtype=torch.float64)
    ref, _ = R.conv_ref(_grid(dz, pad), R.join(dh, dl), 9, w + 2 * pad, add.shape[0], dil=dil, addend=add)
    exp = torch.nn.grad.conv2d_input((N, cin, h, w), wt, dz, padding=dil, dilation=dil) + _interior(add, N, h, w, pad)
    torch.testing.assert_close(_interior(ref, N, h, w, pad), exp, rtol=1e-12, atol=1e-12)


def _s2d(x):
    return torch.cat([x[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=1)


def test_s2d_refs_are_stride2_autograd():
    """The s2d rearrangement's backward (d2s_backward_ref), the mirrored-window input gradient (conv_ref on dgrad_pack_s2d read
    wp + 1 rows further) and the 2x2-window weight gradient (wgrad_ref, taps 4) == autograd of the stride-2 3x3, at odd H2, W2."""
    N, C, cout, H2, W2, pad = 2, 8, 16, 9, 11, 2
    H4, W4 = (H2 + 1) // 2, (W2 + 1) // 2
    x = torch.randn(N, C, H2, W2, generator=_g(12), dtype=torch.float64, requires_grad=True)
    s = _s2d(F.pad(x, (0, W2 % 2, 0, H2 % 2)))
    gs = torch.randn(s.shape, generator=_g(13), dtype=torch.float64)
    s.backward(gs)
    got = R.d2s_backward_ref(_grid(gs, pad), N, C, H2, W2, pad)
    assert torch.equal(got, x.grad.permute(0, 2, 3, 1))
    # the stride-2 3x3 over the s2d grid
    wt = torch.randn(cout, C, 3, 3, generator=_g(14)).to(torch.bfloat16).double()
    xe = torch.randn(N, C, 2 * H4, 2 * W4, generator=_g(15), dtype=torch.float64)
    dz = torch.randn(N, cout, H4, W4, generator=_g(16), dtype=torch.float64)
    wp, rows = W4 + 2 * pad, N * (H4 + 2 * pad) * (W4 + 2 * pad)
    hi, lo = dgrad_pack_s2d(wt.float())
    dzr = _grid(dz, pad)
    ref, _ = R.conv_ref(dzr[wp + 1:], R.join(hi, lo), 4, wp, rows - wp - 1)
    dS = torch.zeros(rows, 4 * C, dtype=torch.float64)
    dS[:rows - wp - 1] = ref
    exp = torch.nn.grad.conv2d_input(xe.shape, wt, dz, stride=2, padding=1)
    torch.testing.assert_close(R.d2s_backward_ref(dS, N, C, 2 * H4, 2 * W4, pad), exp.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    g4, _ = R.wgrad_ref(dzr, _grid(_s2d(xe), pad), rows, wp, 4, cout, 4 * C)
    torch.testing.assert_close(s2d_grad_to_3x3(g4, C), torch.nn.grad.conv2d_weight(xe, wt.shape, dz, stride=2, padding=1),
                               rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dil", [1, 2])
def test_wgrad_ref_is_conv2d_weight(dil):
    N, cin, cout, h, w, pad = 2, 8, 16, 7, 9, 2
    x = torch.randn(N, cin, h, w, generator=_g(17), dtype=torch.float64)
    dz = torch.randn(N, cout, h, w, generator=_g(18), dtype=torch.float64)
    ref, bound = R.wgrad_ref(_grid(dz, pad), _grid(x, pad), N * (h + 2 * pad) * (w + 2 * pad), w + 2 * pad, 9, cout, cin, dil=dil)
    exp = torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), dz, padding=dil, dilation=dil)
    torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)
    assert (bound > 0).all()


def test_stem_wgrad_ref_is_conv2d_weight():
    img = torch.randn(2, 3, 37, 50, generator=_g(19))
    H2, W2 = 19, 25
    dz = torch.randn(2, 32, H2, W2, generator=_g(20))
    hi, lo = split_bf16(_grid(dz, 1))
    ref, _ = R.stem_wgrad_ref(img, (hi, lo))
    exp = torch.nn.grad.conv2d_weight(img.double(), (32, 3, 3, 3), _interior(R.join(hi, lo), 2, H2, W2, 1), stride=2, padding=1)
    torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)


def test_grad_pack_ref_borders_and_nonfinite():
    g = torch.randn(2, 16, 5, 7, generator=_g(21))
    g[0, 3, 1, 2], g[1, 0, 4, 6], g[1, 15, 0, 0] = float("nan"), float("inf"), -float("inf")
    hi, lo = R.grad_pack_ref(g, 2, 32)
    full = (hi.float() + lo.float()).reshape(2, 9, 11, 32)
    assert not full[:, :2].any() and not full[:, :, :2].any() and not full[..., 16:].any()
    assert torch.isnan(full[0, 3, 4, 3]) and hi.reshape(2, 9, 11, 32)[1, 6, 8, 0] == float("inf")
    assert hi.reshape(2, 9, 11, 32)[1, 2, 2, 15] == -float("inf")


# ---- planted defects: each checker rejects what the relative-L2 bar accepts ---------------------------------------------------
def test_checker_rejects_a_one_row_shift_in_the_upsampling_window():
    N, h, w, pad, k = 1, 120, 160, 2, 16
    ph, pw = h // k, w // k
    y, x = torch.meshgrid(torch.arange(h + 2 * pad, dtype=torch.float64), torch.arange(w + 2 * pad, dtype=torch.float64),
                          indexing="ij")
    smooth = torch.sin(0.02 * y + 0.3)[..., None] * torch.cos(0.03 * x)[..., None] * torch.linspace(1, 2, 32, dtype=torch.float64)
    g = torch.zeros(N * (h + 2 * pad) * (w + 2 * pad), 320, dtype=torch.float64)
    g[:, 288:] = smooth.reshape(-1, 32)
    ref, bound = R.spp_upsample_bwd_ref(g, 288, N, h, w, pad, ph, pw)
    R.check("upsample", ref.float(), ref, bound)
    shifted = g.reshape(N, h + 2 * pad, w + 2 * pad, 320).roll(-1, dims=1).reshape(g.shape)   # the window one row too low
    bad, _ = R.spp_upsample_bwd_ref(shifted, 288, N, h, w, pad, ph, pw)
    assert _rel(bad, ref) < 2e-2
    with pytest.raises(AssertionError, match="upsample"):
        R.check("upsample", bad.float(), ref, bound)


def test_checker_rejects_a_pool_term_in_the_remainder_band():
    N, h, w, pad = 2, 67, 131, 2
    g = torch.randn(N * (h + 2 * pad) * (w + 2 * pad), 320, generator=_g(22))
    dpools = [torch.randn(N * (h // k) * (w // k), 128, generator=_g(k)) for k in (64, 32, 16, 8)]
    ref, bound = R.spp_pool_bwd_ref(g, 64, N, h, w, pad, dpools)
    got = ref.float().clone()
    R.check("pool", got, ref, bound)
    got[0, h - 1, 5] += dpools[3][(h // 8 - 1) * (w // 8)] / 64                         # branch4's last cell row leaks one row down
    assert _rel(got, ref) < 2e-2
    with pytest.raises(AssertionError, match="pool"):
        R.check("pool", got, ref, bound)


def _bn_case(seed):
    N, C, h, w, pad = 2, 32, 9, 11, 1
    gen = _g(seed)
    rows = N * (h + 2 * pad) * (w + 2 * pad)
    x = torch.randn(rows, C, generator=gen) * 2 + 0.5
    inner = R.interior_mask(N, h + 2 * pad, w + 2 * pad, pad)
    mean = x[inner].mean(0)
    invstd = 1.0 / torch.sqrt(x[inner].var(0, unbiased=False) + 1e-5)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.2
    xh = (x - mean) * invstd
    g = torch.randn(rows, C, generator=gen) + 0.5 * xh                                  # correlated with xhat: mean g' xhat != 0
    return (N, h + 2 * pad, w + 2 * pad, pad, C), x, mean, invstd, gamma, beta, g


def test_checker_rejects_a_dropped_xhat_term():
    grid, x, mean, invstd, gamma, beta, g = _bn_case(23)
    r = R.bn_backward_ref(x, grid, mean, invstd, gamma, beta, False, g)
    ref, bound = r["dx"]
    inner = R.interior_mask(*grid[:4])
    n = int(inner.sum())
    xh = ((x - mean) * invstd).double()
    bad = ref + gamma.double() * invstd.double() * xh * r["dgamma"][0] / n * inner[:, None]
    R.check("bn dx", ref.float(), ref, bound)
    with pytest.raises(AssertionError, match="bn dx"):
        R.check("bn dx", bad.float(), ref, bound)


def test_checker_rejects_a_mask_flip_off_the_margin():
    grid, x, mean, invstd, gamma, beta, g = _bn_case(24)
    r = R.bn_backward_ref(x, grid, mean, invstd, gamma, beta, True, g)
    ref, bound = r["dx"]
    assert r["marginal"] == 0
    inner = R.interior_mask(*grid[:4])
    t = ((x - mean) * invstd).double() * gamma.double() + beta.double()
    t[~inner] = 0
    row, c = divmod(int(torch.argmin(t)), grid[4])                                       # the most negative pre-ReLU value
    mask = (t > 0) & inner[:, None]
    mask[row, c] = True                                                                  # flipped: the gradient passes there
    bad = R.bn_backward_ref(x, grid, mean, invstd, gamma, beta, True, g, mask=mask)["dx"][0]
    assert _rel(bad, ref) < 2e-2
    with pytest.raises(AssertionError, match="bn dx"):
        R.check("bn dx", bad.float(), ref, bound)


def test_marginal_positions_accept_either_mask():
    """A pre-ReLU value within the fp32 rounding of 0 may go either way: the bound takes both (and what they move the means)."""
    grid, x, mean, invstd, gamma, beta, g = _bn_case(25)
    inner = R.interior_mask(*grid[:4])
    row = int(inner.nonzero()[3])
    x[row, 0] = mean[0] - beta[0] / gamma[0] / invstd[0]                              # t within rounding of 0
    r = R.bn_backward_ref(x, grid, mean, invstd, gamma, beta, True, g)
    assert r["marginal"] >= 1
    ref, bound = r["dx"]
    t = ((x - mean) * invstd).double() * gamma.double() + beta.double()
    for flip in (False, True):
        mask = (t > 0) & inner[:, None]
        mask[row, 0] = flip
        got = R.bn_backward_ref(x, grid, mean, invstd, gamma, beta, True, g, mask=mask)
        R.check("bn dx", got["dx"][0].float(), ref, bound)
        R.check("bn dbeta", got["dbeta"][0].float(), *r["dbeta"])


def test_checker_rejects_a_swapped_s2d_phase():
    N, C, H2, W2, ipad = 2, 8, 9, 11, 2
    H4, W4 = 5, 6
    gs = torch.randn(N * (H4 + 2 * ipad) * (W4 + 2 * ipad), 4 * C, generator=_g(26))
    ref = R.d2s_backward_ref(gs, N, C, H2, W2, ipad)
    swapped = torch.cat([gs[:, :C], gs[:, 2 * C:3 * C], gs[:, C:2 * C], gs[:, 3 * C:]], dim=1)
    R.check("d2s", ref.float(), ref, torch.zeros_like(ref))
    with pytest.raises(AssertionError, match="d2s"):
        R.check("d2s", R.d2s_backward_ref(swapped, N, C, H2, W2, ipad).float(), ref, torch.zeros_like(ref))


def test_checker_rejects_a_dropped_lo_plane():
    """A 1x1 dgrad (the SPP branches' 32 -> 128) whose weights lost their lo plane: relative L2 ~ 2^-10, far under 2e-2."""
    rows, cin, cout = 300, 32, 128
    hx, lx = split_bf16(torch.randn(rows, cin, generator=_g(27)))
    hw, lw = split_bf16(torch.randn(1, cout, cin, generator=_g(28)) * 0.2)
    ref, bound = R.conv_ref(R.join(hx, lx), R.join(hw, lw), 1, 3, rows)
    R.check("conv", ref.float(), ref, bound)
    bad, _ = R.conv_ref(R.join(hx, lx), hw.double(), 1, 3, rows)
    assert _rel(bad.float(), ref) < 2e-2
    with pytest.raises(AssertionError, match="conv"):
        R.check("conv", bad.float(), ref, bound)


def test_checker_rejects_a_nan_and_a_nonzero_border():
    ref = torch.zeros(4, 3, dtype=torch.float64)
    bound = torch.ones_like(ref)
    bound[0] = 0                                                                          # a border row: exact zero
    got = ref.clone().float()
    assert R.check("ok", got, ref, bound) == 0
    got[1, 1] = float("nan")
    with pytest.raises(AssertionError):
        R.check("nan", got, ref, bound)
    got = ref.clone().float()
    got[0, 2] = 1e-30
    with pytest.raises(AssertionError):
        R.check("border", got, ref, bound)
