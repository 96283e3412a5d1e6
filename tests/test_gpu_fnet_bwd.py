"""-m gpu: every launch of the F-Net backward (magnet_amd/train_fnet.py) on its own, pointwise against its fp64 restatement in
tests/fnet_bwd_ref.py, at the edges where these kernels could go wrong: idle threads and two channel passes in the BN reductions,
fewer positions than stage-1 workgroups, channel-slice views, the SPP remainder bands and one-cell upsampling, odd grids, the
dilated / space-to-depth / 1x1 weight-gradient windows, and conv_mfma's addend, out_ld and mirrored-window forms.  Buffers the
kernels must not touch (borders, channels outside a slice, rows past the grid) hold sentinels or NaN."""
import pytest
import torch

from magnet_amd import lib
from magnet_amd.convnet import split_bf16
from magnet_amd.planes import pack_taps
from magnet_amd.train_fnet import dgrad_pack, dgrad_pack_s2d
from tests import fnet_bwd_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bordered(N, h, w, pad, C, gen, scale=1.0, fill=0.0):
    """(N*(h+2pad)*(w+2pad), C) fp32 rows: random interior, `fill` on the border."""
    x = torch.full((N, h + 2 * pad, w + 2 * pad, C), fill)
    x[:, pad:pad + h, pad:pad + w] = torch.randn(N, h, w, C, generator=gen) * scale
    return x.reshape(-1, C)


def _planes(x, gpu):
    hi, lo = split_bf16(x.float().contiguous())
    return hi.to(gpu), lo.to(gpu)


# ---- bn_train_backward ----------------------------------------------------------------------------------------------------------
_BN_GRIDS = {2: (2, 1, 1), 10: (2, 1, 5), 1000: (2, 20, 25), 70131: (3, 97, 241)}       # P -> (N, h, w); 70131 % 256 != 0


@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("P", sorted(_BN_GRIDS))
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [32, 96, 128, 320])
def test_bn_train_backward(hip_lib, gpu, C, relu, P, pad):
    N, h, w = _BN_GRIDS[P]
    hp, wp = h + 2 * pad, w + 2 * pad
    rows = N * hp * wp
    gen = _g(C * 7 + P + pad)
    inner = R.interior_mask(N, hp, wp, pad)
    xv = torch.randn(rows, C, generator=gen) * 2 + 0.3
    mean = xv[inner].mean(0)
    invstd = 1.0 / torch.sqrt(xv[inner].var(0, unbiased=False) + 1e-5)
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen) * 0.3
    gv = torch.randn(rows, C, generator=gen) + 0.3 * (xv - mean) * invstd
    xb = torch.full((rows, C + 16), NAN); xb[:, 8:8 + C] = xv; xb[~inner] = NAN           # border rows and other channels: NaN
    gb = torch.full((rows, C + 8), NAN); gb[:, :C] = gv; gb[~inner] = NAN
    xb, gb = xb.to(gpu), gb.to(gpu)
    x, g = xb[:, 8:8 + C], gb[:, :C]
    dxh = torch.full((rows, C + 24), 7.0, dtype=torch.bfloat16, device=gpu); dxl = dxh.clone()
    dgamma, dbeta = torch.full((C,), NAN, device=gpu), torch.full((C,), NAN, device=gpu)
    work = torch.empty((lib.BN_BLOCKS * 2 + 2) * C, dtype=torch.float64, device=gpu)
    dev = [t.to(gpu) for t in (mean, invstd, gamma, beta)]
    lib.bn_train_backward(x, (N, hp, wp, pad, C), *dev, relu, g, dgamma, dbeta, (dxh[:, 8:8 + C], dxl[:, 8:8 + C]), work)
    r = R.bn_backward_ref(x, (N, hp, wp, pad, C), *dev, relu, g)
    got = R.join(dxh[:, 8:8 + C], dxl[:, 8:8 + C])
    worst = max(R.check("dx", got, *r["dx"]), R.check("dgamma", dgamma, *r["dgamma"]), R.check("dbeta", dbeta, *r["dbeta"]))
    assert (dxh[:, :8] == 7.0).all() and (dxh[:, 8 + C:] == 7.0).all() and (dxl[:, 8 + C:] == 7.0).all()   # outside the slice
    print(f"bn_train_backward C {C} relu {relu} P {P} pad {pad}: worst ratio {worst:.3f} ({r['marginal']} marginal)")


def test_bn_backward_mask_is_the_forward_output(hip_lib, gpu):
    """The backward's recomputed ReLU mask equals bn_train's forward output > 0 bit for bit, at pre-ReLU values planted exactly
    on 0, -0.0 and +- the smallest subnormal (the affine of channels 0..3 is exact), and at random values elsewhere."""
    N, h, w, pad, C = 2, 6, 7, 1, 32
    hp, wp = h + 2 * pad, w + 2 * pad
    rows = N * hp * wp
    gen = _g(3)
    inner = R.interior_mask(N, hp, wp, pad)
    x = torch.randn(rows, C, generator=gen)
    mean, invstd = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen) * 0.1
    tiny = 2.0 ** -149
    mean[:4], invstd[:4], gamma[:4] = 0.0, 1.0, 1.0
    gamma[2] = 2.0 ** -100
    beta[:4] = torch.tensor([0.0, -3.0, 0.0, -tiny])
    ii = inner.nonzero().flatten()
    plant = {0: [0.0, -0.0, tiny, -tiny, 1.0, -1.0], 1: [3.0, 3.0, 3.0000002, 2.9999998],
             2: [2.0 ** -49, -(2.0 ** -49), 0.0, 2.0 ** -48], 3: [2.0 ** -148, 2.0 ** -149, 0.0, 2.0 ** -147]}
    for c, vals in plant.items():
        for j, v in enumerate(vals):
            x[ii[j], c] = v
    g = torch.randn(rows, C, generator=gen).abs() + 1.0                                   # |g| >= 1: a flip moves dx by gamma invstd
    dev = [t.to(gpu) for t in (x, mean, invstd, gamma, beta, g)]
    xg, mg, ig, gg, bg, gradg = dev
    grid = (N, hp, wp, pad, C)
    out = torch.full((rows, C), NAN, device=gpu)
    work = torch.empty(lib.BN_BLOCKS * C * 2, dtype=torch.float64, device=gpu)
    lib.bn_train(xg, grid, mg, ig, work, gg, bg, 1e-5, 0.1, relu=True, out_f32=out, stats=False)
    fwd_mask = (out > 0).cpu()
    assert fwd_mask[ii[2], 0] and not fwd_mask[ii[0], 0] and not fwd_mask[ii[1], 0] and not fwd_mask[ii[3], 0]
    dxh = torch.empty((rows, C), dtype=torch.bfloat16, device=gpu); dxl = torch.empty_like(dxh)
    dgamma, dbeta = torch.empty(C, device=gpu), torch.empty(C, device=gpu)
    wb = torch.empty((lib.BN_BLOCKS * 2 + 2) * C, dtype=torch.float64, device=gpu)
    lib.bn_train_backward(xg, grid, mg, ig, gg, bg, True, gradg, dgamma, dbeta, (dxh, dxl), wb)
    r = R.bn_backward_ref(xg, grid, mg, ig, gg, bg, True, gradg, mask=fwd_mask)
    R.check("dx (forward mask)", R.join(dxh, dxl), *r["dx"])
    R.check("dbeta (forward mask)", dbeta, *r["dbeta"])
    R.check("dgamma (forward mask)", dgamma, *r["dgamma"])


# ---- SPP ------------------------------------------------------------------------------------------------------------------------
_SPP_SHAPES = [(64, 64), (120, 160), (67, 131)]


@pytest.mark.parametrize("hw", _SPP_SHAPES)
@pytest.mark.parametrize("slot,k", [(0, 64), (1, 32), (2, 16), (3, 8)])
def test_spp_upsample_backward(hip_lib, gpu, hw, slot, k):
    h, w = hw
    N, pad = 2, 2
    ph, pw = h // k, w // k
    off = 288 - 32 * slot
    gen = _g(h + k)
    rows = N * (h + 2 * pad) * (w + 2 * pad)
    g = torch.full((rows, 320), NAN)
    g[:, off:off + 32] = _bordered(N, h, w, pad, 32, gen, fill=NAN)                     # only the interior of the slice is read
    g = g.to(gpu)
    dq = torch.full((N * ph * pw + 3, 32), 5.0, device=gpu)
    lib.spp_upsample_backward(g, off, N, h, w, pad, ph, pw, dq)
    ref, bound = R.spp_upsample_bwd_ref(g, off, N, h, w, pad, ph, pw)
    worst = R.check(f"upsample k {k}", dq[:N * ph * pw], ref, bound)
    assert (dq[N * ph * pw:] == 5.0).all()
    print(f"spp_upsample_backward {h}x{w} k {k} (cells {ph}x{pw}): worst ratio {worst:.3f}")


@pytest.mark.parametrize("hw", _SPP_SHAPES)
def test_spp_pool_backward(hip_lib, gpu, hw):
    h, w = hw
    N, pad = 2, 2
    gen = _g(h * w)
    rows = N * (h + 2 * pad) * (w + 2 * pad)
    g = torch.full((rows, 320), NAN)
    g[:, 64:192] = _bordered(N, h, w, pad, 128, gen, fill=NAN)
    g = g.to(gpu)
    dpools = [(torch.randn(N * (h // k) * (w // k), 128, generator=gen) * k).to(gpu) for k in (64, 32, 16, 8)]
    out = torch.full((rows, 128), 9.0, device=gpu)
    lib.spp_pool_backward(g, 64, N, h, w, pad, dpools, out)
    ref, bound = R.spp_pool_bwd_ref(g, 64, N, h, w, pad, dpools)
    grid = out.reshape(N, h + 2 * pad, w + 2 * pad, 128)
    worst = R.check("pool", grid[:, pad:pad + h, pad:pad + w], ref, bound)
    band = bound == 0
    assert band.any() == (h % 8 != 0 or w % 8 != 0)
    assert torch.equal(grid[:, pad:pad + h, pad:pad + w][band], ref[band].float())   # the remainder band: the concat slice
    inner = R.interior_mask(N, h + 2 * pad, w + 2 * pad, pad).to(gpu)
    assert (out[~inner] == 9.0).all()                                                    # border rows untouched
    print(f"spp_pool_backward {h}x{w}: worst ratio {worst:.3f}, {int(band[..., 0].sum())} remainder positions bit-exact")


# ---- fnet_grad_pack, d2s_backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld", [(16, 32), (64, 64)])
def test_fnet_grad_pack(hip_lib, gpu, C, ld):
    N, h, w, pad = 2, 65, 81, 2                                                          # H/4, W/4 of a 257 x 321 input
    g = torch.randn(N, C, h, w, generator=_g(C))
    g[0, 1, 0, 0], g[1, C - 1, h - 1, w - 1], g[0, 0, 7, 3] = NAN, float("inf"), -float("inf")
    g[1, 2, 5, 5] = 3.4e38                                                               # finite in fp32, inf in bf16
    rows = N * (h + 2 * pad) * (w + 2 * pad)
    hi = torch.full((rows + 5, ld), 7.0, dtype=torch.bfloat16, device=gpu); lo = hi.clone()
    lib.fnet_grad_pack(g.to(gpu), hi, lo, pad)
    eh, el = R.grad_pack_ref(g, pad, ld)
    R.check_planes_exact("grad_pack", hi[:rows], lo[:rows], eh, el)
    assert (hi[rows:] == 7.0).all() and (lo[rows:] == 7.0).all()


@pytest.mark.parametrize("ipad", [2, 1])
@pytest.mark.parametrize("H2,W2", [(129, 161), (64, 80), (9, 4)])
def test_fnet_d2s_backward(hip_lib, gpu, H2, W2, ipad):
    N, C = 2, 32
    H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
    gs = _bordered(N, H4, W4, ipad, 4 * C, _g(H2 + W2), fill=NAN).to(gpu)
    out = torch.full((N * (H2 + 2) * (W2 + 2), C), 9.0, device=gpu)
    lib.fnet_d2s_backward(gs, out, N, C, H2, W2, ipad)
    ref = R.d2s_backward_ref(gs, N, C, H2, W2, ipad)
    grid = out.reshape(N, H2 + 2, W2 + 2, C)
    R.check("d2s", grid[:, 1:-1, 1:-1], ref, torch.zeros_like(ref))
    inner = R.interior_mask(N, H2 + 2, W2 + 2, 1).to(gpu)
    assert (out[~inner] == 9.0).all()


# ---- fnet_stem_wgrad ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(1, 25, 19), (2, 37, 51), (2, 64, 64), (2, 257, 321)])   # P = 130 < 256, 988, 2048, 41 538
def test_fnet_stem_wgrad(hip_lib, gpu, N, H, W):
    gen = _g(H * W)
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = torch.randn(N, 3, H, W, generator=gen).to(gpu)
    dz = _planes(_bordered(N, H2, W2, 1, 32, gen), gpu)
    gw = torch.full((32, 3, 3, 3), NAN, device=gpu)
    lib.fnet_stem_wgrad(img, dz, gw, torch.empty(lib.BN_BLOCKS * 864, dtype=torch.float64, device=gpu))
    ref, bound = R.stem_wgrad_ref(img, dz)
    worst = R.check("stem wgrad", gw, ref, bound)
    print(f"fnet_stem_wgrad {N}x{H}x{W} (P {N * H2 * W2}): worst ratio {worst:.3f}")


# ---- wgrad_ex ---------------------------------------------------------------------------------------------------------------------
_WG = {  # name: (taps, dil, cout, cout_valid, cin, x_width, x_off, cin_dst)
    "taps9_dil1": (9, 1, 64, 64, 64, 64, 0, 0),
    "taps9_dil2": (9, 2, 128, 128, 128, 128, 0, 0),
    "taps4_s2d": (4, 1, 64, 64, 128, 128, 0, 0),
    "taps1_cout_valid": (1, 1, 32, 16, 128, 128, 0, 0),
    "taps9_cin320": (9, 1, 128, 128, 320, 320, 0, 0),
    "taps9_view_of_320": (9, 2, 128, 128, 128, 320, 64, 0),
    "taps1_view_cin_dst": (1, 1, 128, 128, 64, 320, 0, 64),
}


@pytest.mark.parametrize("case", sorted(_WG))
def test_wgrad_ex(hip_lib, gpu, case):
    taps, dil, cout, cv, cin, xw, xoff, cdst = _WG[case]
    N, h, w, pad = 2, 40, 44, 2                                                          # 4224 rows: three 2048-row chunks
    wp, rows = w + 2 * pad, N * (h + 2 * pad) * (w + 2 * pad)
    gen = _g(len(case) * 13 + cin)
    dyv = _bordered(N, h, w, pad, cout, gen)
    if cv < cout:
        dyv[:, cv:] = 0                                                                  # as fnet_grad_pack leaves them
    dy = _planes(dyv, gpu)
    xv = _bordered(N, h, w, pad, xw, gen)
    xf = _planes(xv, gpu)
    x = (xf[0][:, xoff:xoff + cin], xf[1][:, xoff:xoff + cin])
    k = {9: 3, 4: 2, 1: 1}[taps]
    gw = torch.full((cv, cdst + cin + 8, k, k), 3.0, device=gpu)
    lib.wgrad_ex(dy[0], dy[1], x[0], x[1], rows, wp, taps, cout, cin, gw, dil=dil, cin_dst=cdst, cout_valid=cv)
    ref, bound = R.wgrad_ref(R.join(*dy), R.join(*x), rows, wp, taps, cout, cin, dil=dil)
    worst = R.check(f"wgrad_ex {case}", gw[:, cdst:cdst + cin], ref[:cv], bound[:cv])
    assert (gw[:, :cdst] == 3.0).all() and (gw[:, cdst + cin:] == 3.0).all()
    print(f"wgrad_ex {case}: worst ratio {worst:.3f}")


# ---- conv_mfma as the backward calls it -----------------------------------------------------------------------------------------
def _grid_rows(N, h, w, pad, gpu):
    return R.interior_mask(N, h + 2 * pad, w + 2 * pad, pad).to(gpu)


def test_conv_dgrad_dilated_with_a_320_wide_addend(hip_lib, gpu):
    """layer4's input gradient: a flipped, transposed pack at dilation 2, + the fp32 addend read with row pitch 320."""
    N, h, w, pad, c = 2, 30, 41, 2, 128
    wp, rows = w + 2 * pad, N * (h + 2 * pad) * (w + 2 * pad)
    gen = _g(41)
    dz = _planes(_bordered(N, h, w, pad, c, gen), gpu)
    wt = torch.randn(c, c, 3, 3, generator=gen) * 0.05
    hi, lo = dgrad_pack(wt.to(gpu))
    add = torch.randn(rows, 320, generator=gen).to(gpu)
    out = torch.full((rows, c), NAN, device=gpu)
    lib.conv_mfma(dz[0], dz[1], c, c, hi, lo, torch.zeros(c, device=gpu), 9, wp, False, rows, out_f32=out, dil=2, addend=add)
    ref, bound = R.conv_ref(R.join(*dz), R.join(hi, lo), 9, wp, rows, dil=2, addend=add[:, :c])
    inner = _grid_rows(N, h, w, pad, gpu)
    worst = R.check("dgrad dil 2 + addend", out[inner], ref[inner], bound[inner])
    print(f"conv_mfma dgrad dil 2 + addend ld 320: worst ratio {worst:.3f}")


def test_conv_dgrad_into_the_concat_slices(hip_lib, gpu):
    """lastconv.0's input gradient: three launches (128, 128, 64 channels) written into a 320-wide fp32 buffer with out_ld 320."""
    N, h, w, pad = 2, 21, 33, 2
    wp, rows = w + 2 * pad, N * (h + 2 * pad) * (w + 2 * pad)
    gen = _g(42)
    dz = _planes(_bordered(N, h, w, pad, 128, gen), gpu)
    wf = (torch.randn(128, 320, 3, 3, generator=gen) * 0.03).to(gpu)
    g_cat = torch.full((rows, 320), NAN, device=gpu)
    refs, bounds = [], []
    for c_lo, c_hi in ((0, 128), (128, 256), (256, 320)):
        hi, lo = dgrad_pack(wf[:, c_lo:c_hi])
        lib.conv_mfma(dz[0], dz[1], 128, 128, hi, lo, torch.zeros(c_hi - c_lo, device=gpu), 9, wp, False, rows,
                      out_f32=g_cat[:, c_lo:], out_ld=320)
        r, b = R.conv_ref(R.join(*dz), R.join(hi, lo), 9, wp, rows)
        refs.append(r); bounds.append(b)
    inner = _grid_rows(N, h, w, pad, gpu)
    worst = R.check("dgrad concat slices", g_cat[inner], torch.cat(refs, 1)[inner], torch.cat(bounds, 1)[inner])
    print(f"conv_mfma dgrad into the 320-wide concat (out_ld 320): worst ratio {worst:.3f}")


def test_conv_dgrad_mirrored_s2d_window(hip_lib, gpu):
    """layer2.0's input gradient: the phase-0 1x1 downsample into a 4C-wide buffer (out_ld 4C), then the mirrored 2x2 window read
    from row wp + 1 over rows - wp - 1 rows, with that buffer as the addend (row pitch 4C)."""
    N, h, w, pad, C, cout = 2, 31, 40, 2, 32, 64
    wp, rows = w + 2 * pad, N * (h + 2 * pad) * (w + 2 * pad)
    gen = _g(43)
    dz1 = _planes(_bordered(N, h, w, pad, cout, gen), gpu)
    dzd = _planes(_bordered(N, h, w, pad, cout, gen), gpu)
    w1 = (torch.randn(cout, C, 3, 3, generator=gen) * 0.1).to(gpu)
    wd = (torch.randn(cout, C, 1, 1, generator=gen) * 0.1).to(gpu)
    short = torch.zeros((rows, 4 * C), device=gpu)
    hd, ld = dgrad_pack(wd)
    lib.conv_mfma(dzd[0], dzd[1], cout, cout, hd, ld, torch.zeros(C, device=gpu), 1, wp, False, rows, out_f32=short, out_ld=4 * C)
    inner = _grid_rows(N, h, w, pad, gpu)
    rs, bs = R.conv_ref(R.join(*dzd), R.join(hd, ld), 1, wp, rows)
    w_sh = R.check("downsample phase 0", short[inner, :C], rs[inner], bs[inner])
    assert not short[:, C:].any()                                                        # phases 1-3 untouched
    hi, lo = dgrad_pack_s2d(w1)
    dS = torch.full((rows, 4 * C), NAN, device=gpu)
    lib.conv_mfma(dz1[0][wp + 1:], dz1[1][wp + 1:], cout, cout, hi, lo, torch.zeros(4 * C, device=gpu), 4, wp, False, rows - wp - 1,
                  out_f32=dS, addend=short)
    ref, bound = R.conv_ref(R.join(*dz1)[wp + 1:], R.join(hi, lo), 4, wp, rows - wp - 1, addend=short)
    inner_s = inner[:rows - wp - 1]
    worst = R.check("mirrored s2d window", dS[:rows - wp - 1][inner_s], ref[inner_s], bound[inner_s])
    print(f"conv_mfma downsample (out_ld 4C) {w_sh:.3f}, mirrored s2d window + addend: worst ratio {worst:.3f}")


def test_conv_dgrad_lastconv2_pack(hip_lib, gpu):
    """lastconv.2's input gradient: the 1x1 pack of the transposed (Fd -> 128) weights padded to 32 input channels (Fd 16)."""
    N, h, w, pad, Fd, Fp = 2, 17, 23, 2, 16, 32
    wp, rows = w + 2 * pad, N * (h + 2 * pad) * (w + 2 * pad)
    gen = _g(44)
    g = torch.randn(N, Fd, h, w, generator=gen).to(gpu)
    dF = (torch.empty((rows, Fp), dtype=torch.bfloat16, device=gpu), torch.empty((rows, Fp), dtype=torch.bfloat16, device=gpu))
    lib.fnet_grad_pack(g, dF[0], dF[1], pad)
    w2 = torch.randn(Fd, 128, 1, 1, generator=gen).to(gpu) * 0.1
    wt = torch.zeros((128, Fp, 1, 1), device=gpu)
    wt[:, :Fd] = w2.transpose(0, 1)
    hi, lo = pack_taps(wt)
    out = torch.full((rows, 128), NAN, device=gpu)
    lib.conv_mfma(dF[0], dF[1], Fp, Fp, hi, lo, torch.zeros(128, device=gpu), 1, wp, False, rows, out_f32=out)
    ref, bound = R.conv_ref(R.join(*dF), R.join(hi, lo), 1, wp, rows)
    worst = R.check("lastconv.2 dgrad", out, ref, bound)                                 # 1x1: every row, borders give 0
    print(f"conv_mfma lastconv.2 dgrad (Fd 16 in 32): worst ratio {worst:.3f}")
