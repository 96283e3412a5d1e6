"""CPU: the fp64 restatements of tests/heads_bwd_ref.py equal torch float64 autograd of the formulas the repository pins to the
reference (tests/stubs.py: magnet_nll_loss, magnet.py: _upsample_depth_torch and GNET, an nn.Sequential mask head), and each checker
rejects a planted defect that a 1e-4 relative-L2 bar on the whole tensor accepts."""
import pytest
import torch
import torch.nn as nn

from magnet_amd.convnet import split_bf16
from magnet_amd.magnet import GNET, _upsample_depth_torch
from tests import fnet_bwd_ref as FR
from tests import heads_bwd_ref as R
from tests.stubs import magnet_nll_loss


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _grid(x_nchw):
    """(B, C, h, w) -> the zero-bordered channel-last rows (B*(h+2)*(w+2), C)."""
    B, C, h, w = x_nchw.shape
    out = torch.zeros((B, h + 2, w + 2, C), dtype=x_nchw.dtype)
    out[:, 1:-1, 1:-1] = x_nchw.permute(0, 2, 3, 1)
    return out.reshape(-1, C)


def _nll_case(seed, n=3, B=2, H=9, W=13, clamp=False):
    gen = _g(seed)
    mu = torch.rand(n, B, 1, H, W, generator=gen) * 3 + 1
    sg = torch.rand(n, B, 1, H, W, generator=gen) * 0.5 + 0.05
    if clamp:
        sg[1, 0, 0, :2, :3] = 1e-6                                                       # var 1e-12: clamped
    preds = torch.cat([mu, sg], 2)
    gt = torch.rand(B, H, W, generator=gen) * 3 + 1
    mask = torch.rand(B, H, W, generator=gen) > 0.3
    return preds, gt, mask


# ---- the restatements against autograd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True])
def test_nll_refs_are_magnet_nll_loss_autograd(clamp):
    """Value and gradient.  Where the clamp applies the kernel uses fp32's 1e-10 (as the reference's fp32 run does) and fp64 autograd
    the double 1e-10: 1.3e-8 apart, so that case compares at 1e-7; its gradient of sigma is exactly 0 in both."""
    preds, gt, mask = _nll_case(1, clamp=clamp)
    gamma, gl = 0.7, 2.5
    r = R.nll_forward_ref(preds, gt, mask, gamma)
    pl = [p.double().requires_grad_(True) for p in preds.unbind(0)]
    loss = magnet_nll_loss(pl, gt.double()[:, None], mask[:, None], gamma=gamma)
    (gl * loss).backward()
    tol = 1e-7 if clamp else 1e-12
    assert float(r["count"]) == float(mask.sum())
    torch.testing.assert_close(r["loss"][0], loss.detach(), rtol=tol, atol=0)
    ref, bound = R.nll_backward_ref(preds, gt, mask, r["count"], gl, gamma)
    torch.testing.assert_close(ref, torch.stack([p.grad for p in pl]), rtol=tol, atol=1e-12)
    assert not ref.transpose(1, 2)[:, :, ~mask].any() and not bound.transpose(1, 2)[:, :, ~mask].any()            # masked: exactly 0
    if clamp:
        assert ref[1, 0, 1, :2, :3].abs().max() == 0 and bound[1, 0, 1, :2, :3].abs().max() == 0
    # per-iteration sums are the unweighted masked sums of the NLL
    for i in range(preds.shape[0]):
        one = magnet_nll_loss([pl[i].detach()], gt.double()[:, None], mask[:, None])
        torch.testing.assert_close(r["sums"][0][i] / r["count"], one, rtol=tol, atol=0)


@pytest.mark.parametrize("B,h,w,n", [(2, 5, 7, 3), (1, 1, 1, 2), (1, 1, 6, 1)])
def test_upsample_ref_is_upsample_autograd(B, h, w, n):
    k = 4
    gen = _g(h * 10 + w)
    depth = torch.rand(n, B, 2, h, w, generator=gen, dtype=torch.float64) + 0.5
    mask = torch.randn(B, 9 * k * k, h, w, generator=gen, dtype=torch.float64) * 3
    gup = torch.randn(n, B, 2, k * h, k * w, generator=gen, dtype=torch.float64)
    d64, m64 = depth.clone().requires_grad_(True), mask.clone().requires_grad_(True)
    sum((_upsample_depth_torch(d64[i], m64, k) * gup[i]).sum() for i in range(n)).backward()
    r = R.upsample_bwd_ref(gup, depth, mask, k)
    torch.testing.assert_close(r["grad_depth"][0], d64.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(r["grad_mask"][0], m64.grad, rtol=1e-11, atol=1e-12)
    # the padded channel-last layout of the HIP training path reads the same logits
    ld, wp = 144, w + 2
    buf = torch.full((B * (h + 2) * wp, ld), float("nan"), dtype=torch.float64)
    lay = ((wp + 1) * ld, (h + 2) * wp * ld, 1, wp * ld, ld)
    R.strided(buf, lay, tuple(mask.shape)).copy_(mask)
    r2 = R.upsample_bwd_ref(gup, depth, buf, k, mask_layout=lay)
    assert torch.equal(r2["grad_mask"][0], r["grad_mask"][0]) and torch.equal(r2["grad_depth"][0], r["grad_depth"][0])
    assert int(R.addressed(buf, lay, tuple(mask.shape)).sum()) == mask.numel()


def _hooked(seq):
    """Run-time capture of every conv's (pre-ReLU) output with retain_grad; the ReLUs made out-of-place."""
    outs = []

    def hook(mod, inp, out):
        out.retain_grad()
        outs.append(out)
    for mod in seq:
        if isinstance(mod, nn.ReLU):
            mod.inplace = False
        if isinstance(mod, nn.Conv2d):
            mod.register_forward_hook(hook)
    return outs


def _planes_of(act):
    return split_bf16(_grid(torch.relu(act.detach()).float()))[0]


def _chain(wt3, outs, dout_ref, B, h, w, k0):
    """Run the three stages on fp64 operands (no split between them) and compare with the retained gradients."""
    W4T, W3T, W2T = R.wt_parts(wt3, k0)
    g = dout_ref
    for wt, hh, o in ((W4T, outs[2], outs[2]), (W3T, outs[1], outs[1]), (W2T, outs[0], outs[0])):
        s = R.dgrad_stage_ref(wt, g, _planes_of(hh), B, h, w)
        assert s["marginal"] == 0
        ref, bound = s["acc"]
        torch.testing.assert_close(ref, _grid(o.grad), rtol=1e-11, atol=1e-13)
        assert (bound > 0).sum() > 0 and not ref.reshape(B, h + 2, w + 2, -1)[:, 0].any()
        g = ref


def test_gauss_and_dgrad_refs_are_gnet_autograd():
    B, h, w, D = 2, 5, 6, 5
    gen = _g(3)
    net = GNET(D + 8).double()
    for p in net.parameters():
        p.data.normal_(generator=gen).mul_(0.3)
    outs = _hooked(net.gnet)
    cost = torch.randn(B, D + 8, h, w, generator=gen, dtype=torch.float64)
    gmm = torch.cat([torch.rand(B, 1, h, w, generator=gen) + 1, torch.rand(B, 1, h, w, generator=gen) * 0.5 + 0.1], 1).double()
    out = net(cost, gmm)
    gg = torch.randn(B, 2, h, w, generator=gen, dtype=torch.float64)
    out.backward(gg)
    o4 = _grid(outs[3].detach())                                                        # the head's output (rows, 2)
    gnet_out = torch.zeros(o4.shape[0], 16, dtype=torch.float64)
    gnet_out[:, :2] = o4
    ref, bound = R.gauss_stage_ref(gg, gnet_out, gmm, B, h, w)
    torch.testing.assert_close(ref[:, :2], _grid(outs[3].grad), rtol=1e-12, atol=1e-14)
    assert not ref[:, 2:].any() and (bound[:, :2][ref[:, :2] != 0] > 0).all()
    wts = [net.gnet[6].weight, net.gnet[4].weight, net.gnet[2].weight]
    W4T = torch.zeros(128, 32, dtype=torch.float64)
    W4T[:, :2] = wts[0].detach()[:, :, 0, 0].T
    wt = torch.cat([W4T.reshape(-1), wts[1].detach()[:, :, 0, 0].T.reshape(-1), wts[2].detach()[:, :, 0, 0].T.reshape(-1)])
    _chain(wt, outs, ref, B, h, w, 32)


def test_dgrad_refs_are_mask_head_autograd():
    B, h, w = 2, 4, 7
    gen = _g(4)
    head = nn.Sequential(nn.Conv2d(16, 128, 3, padding=1), nn.ReLU(True), nn.Conv2d(128, 128, 1), nn.ReLU(True),
                         nn.Conv2d(128, 128, 1), nn.ReLU(True), nn.Conv2d(128, 144, 1)).double()
    for p in head.parameters():
        p.data.normal_(generator=gen).mul_(0.2)
    outs = _hooked(head)
    x = torch.randn(B, 16, h, w, generator=gen, dtype=torch.float64)
    gy = torch.randn(B, 144, h, w, generator=gen, dtype=torch.float64)
    head(x).backward(gy)
    dout = torch.zeros(B * (h + 2) * (w + 2), 160, dtype=torch.float64)
    dout[:, :144] = _grid(gy)
    W4T = torch.zeros(128, 160, dtype=torch.float64)
    W4T[:, :144] = head[6].weight.detach()[:, :, 0, 0].T
    wt = torch.cat([W4T.reshape(-1), head[4].weight.detach()[:, :, 0, 0].T.reshape(-1), head[2].weight.detach()[:, :, 0, 0].T.reshape(-1)])
    _chain(wt, outs, dout, B, h, w, 160)


@pytest.mark.parametrize("taps", [9, 1])
def test_wgrad_ref_is_conv2d_weight(taps):
    B, cin, cout, h, w = 3, 24, 16, 5, 7
    gen = _g(taps)
    x = torch.randn(B, cin, h, w, generator=gen, dtype=torch.float64)
    dz = torch.randn(B, cout, h, w, generator=gen, dtype=torch.float64)
    rows, wp = B * (h + 2) * (w + 2), w + 2
    k = 3 if taps == 9 else 1
    r = R.wgrad_plain_ref(_grid(dz), _grid(x), rows, wp, taps, cout, cin, cin_valid=20)
    exp = torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dz, padding=k // 2)
    torch.testing.assert_close(r["w"][0], exp[:, :20], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["b"][0], dz.sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    if taps == 9:                                                                        # the F-Net restatement's window is the same
        ref9, _ = FR.wgrad_ref(_grid(dz), _grid(x), rows, wp, 9, cout, cin)
        torch.testing.assert_close(r["w"][0], ref9[:, :20], rtol=1e-12, atol=1e-12)
    old = torch.randn(r["w"][0].shape, generator=gen, dtype=torch.float64)
    ra = R.wgrad_plain_ref(_grid(dz), _grid(x), rows, wp, taps, cout, cin, cin_valid=20, old_w=old)
    torch.testing.assert_close(ra["w"][0], exp[:, :20] + old, rtol=1e-12, atol=1e-12)


# ---- planted defects: each checker rejects what the relative-L2 bar accepts ---------------------------------------------------
def test_checker_rejects_a_dropped_wgrad_chunk():
    """Three chunks (P = 2 x 2048 + 32); the output gradient is small (1e-4) in the 32-row ragged tail and input channel 7 is live
    only there.  Dropping that chunk moves the whole gradient by < 1e-4 relative L2 but zeroes column 7."""
    B, h, w = 1, 70, 57
    rows, wp = B * (h + 2) * (w + 2), w + 2
    P, nch = R.wgrad_chunks(rows, wp)
    assert (P, nch) == (4128, 3)
    gen = _g(5)
    dy = torch.randn(rows, 32, generator=gen, dtype=torch.float64) * R.interior_mask(B, h + 2, w + 2, 1)[:, None]
    x = torch.randn(rows, 32, generator=gen, dtype=torch.float64)
    tail0 = wp + 1 + 2 * 2048
    dy[tail0:] *= 1e-4
    x[:tail0, 7] = 0
    ref, bound = R.wgrad_plain_ref(dy, x, rows, wp, 1, 32, 32)["w"]
    R.check("wgrad", ref.float(), ref, bound)
    dy_bad = dy.clone()
    dy_bad[tail0:] = 0                                                                   # the last chunk's partial tile dropped
    bad, _ = R.wgrad_plain_ref(dy_bad, x, rows, wp, 1, 32, 32)["w"]
    assert _rel(bad, ref) < 1e-4
    with pytest.raises(AssertionError, match="wgrad"):
        R.check("wgrad", bad.float(), ref, bound)


def test_checker_rejects_a_border_row_off_by_one():
    """dg_border with y == hp - 2: each image's last interior row is zeroed.  With gradients small there (1e-4 of the rest) the
    whole-tensor change is 1e-5 relative L2."""
    B, h, w = 2, 30, 40
    rows = B * (h + 2) * (w + 2)
    gen = _g(6)
    g = torch.randn(rows, 128, generator=gen, dtype=torch.float64)
    g.reshape(B, h + 2, w + 2, 128)[:, h] *= 1e-4
    wt = torch.randn(128, 128, generator=gen, dtype=torch.float64) * 0.1
    hh = split_bf16(torch.rand(rows, 128, generator=gen))[0]
    s = R.dgrad_stage_ref(wt, g, hh, B, h, w)
    ref, bound = s["planes"]
    R.check("dgrad", ref.float(), ref, bound)
    bad = ref.clone()
    bad.reshape(B, h + 2, w + 2, 128)[:, h] = 0
    assert _rel(bad, ref) < 1e-4
    with pytest.raises(AssertionError, match="dgrad"):
        R.check("dgrad", bad.float(), ref, bound)


def test_checker_rejects_a_first_order_elu_derivative():
    """elu'(o1) = 1 + o1 instead of exp(o1) where o1 <= 0: |o1| <= 0.012 keeps it under 1e-4 relative L2."""
    B, h, w = 2, 20, 30
    gen = _g(7)
    rows = B * (h + 2) * (w + 2)
    gg = torch.randn(B, 2, h, w, generator=gen)
    gmm = torch.cat([torch.rand(B, 1, h, w, generator=gen) + 1, torch.rand(B, 1, h, w, generator=gen) * 0.5 + 0.1], 1)
    out = torch.zeros(rows, 16)
    out[:, 1] = (torch.rand(rows, generator=gen) - 0.5) * 0.024
    ref, bound = R.gauss_stage_ref(gg, out, gmm, B, h, w)
    R.check("gauss", ref.float(), ref, bound)
    bad, _ = R.gauss_stage_ref(gg, out, gmm, B, h, w, elu_prime=lambda o: torch.where(o > 0, torch.ones_like(o), 1 + o))
    assert _rel(bad, ref) < 1e-4
    with pytest.raises(AssertionError, match="gauss"):
        R.check("gauss", bad.float(), ref, bound)


def test_checker_rejects_a_pixel_counted_twice():
    preds, gt, mask = _nll_case(8, n=2, B=2, H=200, W=250)
    q = (0, 100, 120)
    mask[q] = True
    preds[1, 0, 0, 100, 120] = gt[q] + 0.5                                              # a pixel with a larger term than most
    r = R.nll_forward_ref(preds, gt, mask, 0.8)
    sums, bound = r["sums"]
    R.check("nll sums", sums.float(), sums, bound)
    d, var, *_ = R._nll_terms(preds, gt, mask)
    bad = sums + (d[:, 0, 100, 120] ** 2 / (2 * var[:, 0, 100, 120]) + 0.5 * torch.log(var[:, 0, 100, 120]))
    assert _rel(bad, sums) < 1e-4
    with pytest.raises(AssertionError, match="nll sums"):
        R.check("nll sums", bad, sums, bound)
    with pytest.raises(AssertionError, match="count"):
        R.check("nll count", r["count"] + 1, r["count"], torch.zeros(()))


def test_checker_rejects_a_shifted_gather_tap():
    """Pass 2 reading tap 4's partial sum one row too low inside the grid: smooth depth and gradients keep the change at ~1e-5."""
    n, B, h, w, k = 1, 1, 40, 50, 4
    yy = torch.arange(k * h, dtype=torch.float64)[:, None]
    xx = torch.arange(k * w, dtype=torch.float64)[None, :]
    gup = (1 + 1e-4 * yy + 1e-4 * xx).expand(n, B, 2, k * h, k * w).contiguous()
    depth = torch.ones(n, B, 2, h, w, dtype=torch.float64)
    mask = torch.zeros(B, 9 * k * k, h, w, dtype=torch.float64)
    r = R.upsample_bwd_ref(gup, depth, mask, k)
    ref, bound = r["grad_depth"]
    R.check("gather", ref.float(), ref, bound)
    p = torch.full((k * k,), 1.0 / 9, dtype=torch.float64)
    g = gup.reshape(n, B, 2, h, k, w, k).permute(0, 1, 2, 4, 6, 3, 5).reshape(n, B, 2, k * k, h, w)
    part4 = torch.einsum("s,nbcsyx->nbcyx", p, g)
    bad = ref.clone()
    bad[..., :h - 1, :] += part4[..., 1:, :] - part4[..., :h - 1, :]
    assert _rel(bad, ref) < 1e-4
    with pytest.raises(AssertionError, match="gather"):
        R.check("gather", bad.float(), ref, bound)


def test_checker_rejects_a_nan_and_a_write_into_the_padding():
    B, h, w, k = 1, 3, 4, 4
    ld, wp = 160, w + 2
    lay = ((wp + 1) * ld, (h + 2) * wp * ld, 1, wp * ld, ld)
    buf = torch.full((B * (h + 2) * wp, ld), 7.0)
    keep = R.addressed(buf, lay, (B, 9 * k * k, h, w))
    assert int(keep.sum()) == B * 144 * h * w and not keep[:, 144:].any()
    R.check_untouched("grad_mask", buf, keep, 7.0)
    ref = torch.randn(B, 144, h, w, generator=_g(9), dtype=torch.float64)
    R.strided(buf, lay, tuple(ref.shape)).copy_(ref)
    R.check("grad_mask", R.strided(buf, lay, tuple(ref.shape)), ref, ref.abs() * 1e-6 + 1e-30)
    buf[wp + 2, 150] = 0.0                                                               # a padding channel of an interior row
    assert _rel(R.strided(buf, lay, tuple(ref.shape)), ref) < 1e-4                      # the view cannot see it
    with pytest.raises(AssertionError, match="grad_mask"):
        R.check_untouched("grad_mask", buf, keep, 7.0)
    got = R.strided(buf, lay, tuple(ref.shape)).clone()
    got[0, 3, 1, 1] = float("nan")
    with pytest.raises(AssertionError):
        R.check("grad_mask", got, ref, ref.abs() * 1e-6 + 1e-30)


def test_marginal_h_accepts_either_mask_and_nothing_else():
    """The ReLU mask is [h_hi > 0] on the bf16 plane: 0 and -0 close it, normal positives open it, a positive subnormal (a
    flush-to-zero compare reads 0) takes either; a value whose hi rounded to 0 is closed."""
    B, h, w = 1, 2, 3
    rows = B * (h + 2) * (w + 2)
    gen = _g(10)
    g = torch.randn(rows, 128, generator=gen, dtype=torch.float64)
    wt = torch.randn(128, 128, generator=gen, dtype=torch.float64)
    hf = torch.ones(rows, 128)
    inner = R.interior_mask(B, h + 2, w + 2, 1).nonzero().flatten()
    r0 = int(inner[0])
    hf[r0, :5] = torch.tensor([0.0, -0.0, 2.0 ** -133, 2.0 ** -126, 2.0 ** -140])      # 0, -0, subnormal, min normal, hi -> 0
    hh = hf.to(torch.bfloat16)
    s = R.dgrad_stage_ref(wt, g, hh, B, h, w)
    assert s["marginal"] == 1
    ref, bound = s["acc"]
    y = (g @ wt.T)[r0]
    for c in (2,):
        for got in (0.0, float(y[c])):
            R.check("marginal", torch.tensor([got]), ref[r0, c:c + 1], bound[r0, c:c + 1])
    for c, exp in ((0, 0.0), (1, 0.0), (4, 0.0), (3, float(y[3]))):
        assert bound[r0, c] < 1e-3 * abs(float(y[c])) and float(ref[r0, c]) == exp
        wrong = float(y[c]) if exp == 0.0 else 0.0
        with pytest.raises(AssertionError):
            R.check("flip", torch.tensor([wrong]), ref[r0, c:c + 1], bound[r0, c:c + 1])
