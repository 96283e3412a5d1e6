"""-m gpu: every launch of the G-Net / mask-head training backward (magnet_amd/train.py, csrc/train_bwd.hip) on its own, pointwise
against its fp64 restatement in tests/heads_bwd_ref.py, at the edges where these kernels could go wrong: one, several and ragged
2048-row wgrad chunks, B > 1 grids whose 3x3 taps reach the neighbouring image, the production channel counts (8 of which 2 valid,
144 in a 160-wide plane, 256 through a column-offset view), accumulate; dgrad tiles past the last row and both first-stage forms;
loss grids past one pass of the 256 x 256 threads, 1 and 16 iterations, the variance clamp and a fully masked image; one-pixel and
odd upsampling grids with logits of +-80.  Buffers the kernels must not touch hold sentinels or NaN."""
import ctypes

import pytest
import torch

from magnet_amd import lib
from magnet_amd.convnet import split_bf16
from tests import heads_bwd_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = 3.0


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _planes(x, gpu, extra=0, fill=NAN):
    """split bf16 planes of x (rows, C) on the device, with `extra` sentinel rows past the end."""
    hi, lo = split_bf16(x.float().contiguous())
    if extra:
        pad = torch.full((extra, x.shape[1]), fill, dtype=torch.bfloat16)
        hi, lo = torch.cat([hi, pad]), torch.cat([lo, pad])
    return hi.to(gpu), lo.to(gpu)


# ---- wgrad --------------------------------------------------------------------------------------------------------------------
_WG_GRIDS = {"sub_chunk": (1, 20, 30), "one_chunk": (2, 24, 39), "two_ragged": (3, 21, 37), "three_tail32": (1, 70, 57),
             "three_b4": (4, 30, 39)}
_WG_LAYERS = {  # name: (taps, cout, cout_valid, dy_ld, cin, x_ld, x_off, cin_valid, cin_dst, cin_total, accumulate)
    "gnet_last": (1, 8, 2, 32, 128, 128, 0, 128, 0, 128, True),
    "mask_last": (1, 144, 144, 160, 128, 128, 0, 128, 0, 128, False),
    "mid_1x1": (1, 128, 128, 128, 128, 128, 0, 128, 0, 128, True),
    "first_x_d3": (9, 128, 128, 128, 256, 288, 32, 256, 5, 261, False),
    "first_cost": (9, 128, 128, 128, 32, 32, 0, 5, 0, 261, True),
}


@pytest.mark.parametrize("layer", sorted(_WG_LAYERS))
@pytest.mark.parametrize("grid", sorted(_WG_GRIDS))
def test_wgrad(hip_lib, gpu, grid, layer):
    B, h, w = _WG_GRIDS[grid]
    taps, cout, cv, dy_ld, cin, x_ld, x_off, ci, cdst, ctot, acc = _WG_LAYERS[layer]
    rows, wp = B * (h + 2) * (w + 2), w + 2
    gen = _g(rows + cout + cin)
    inner = R.interior_mask(B, h + 2, w + 2, 1)
    dyv = torch.full((rows, dy_ld), NAN)                                                 # channels past cout: never read
    dyv[:, :cout] = torch.randn(rows, cout, generator=gen) * inner[:, None]               # zero on border rows (the contract)
    xv = torch.full((rows, x_ld), NAN)
    xv[:, x_off:x_off + cin] = torch.randn(rows, cin, generator=gen)                      # live data on border rows and pad channels
    dy = _planes(dyv, gpu, extra=7)
    xf = _planes(xv, gpu, extra=7)
    x = (xf[0][:, x_off:x_off + cin], xf[1][:, x_off:x_off + cin])
    k = 3 if taps == 9 else 1
    gw = torch.full((cv + 3, ctot, k, k), SENT, device=gpu)                             # rows past cout_valid: sentinel
    gb = torch.full((cout + 4,), SENT, device=gpu)
    old_w = old_b = None
    if acc:
        gw[:cv, cdst:cdst + ci] = torch.randn(cv, ci, k, k, generator=gen).to(gpu)
        gb[:cv] = torch.randn(cv, generator=gen).to(gpu)
        old_w, old_b = gw[:cv, cdst:cdst + ci].clone(), gb[:cv].clone()
    lib.wgrad(dy[0][:, :cout], dy[1][:, :cout], x[0], x[1], rows, wp, taps, cout, cin, gw[:cv], cin_dst=cdst, cout_valid=cv,
              cin_valid=ci, grad_b=gb, accumulate=acc)
    r = R.wgrad_plain_ref(R.join(*dy)[:rows], R.join(*x)[:rows], rows, wp, taps, cout, cin, cout_valid=cv, cin_valid=ci,
                          old_w=old_w, old_b=old_b)
    ww = R.check(f"wgrad {layer} {grid} w", gw[:cv, cdst:cdst + ci], *r["w"])
    wb = R.check(f"wgrad {layer} {grid} b", gb[:cv], *r["b"])
    keep = torch.zeros(gw.shape, dtype=torch.bool, device=gpu)
    keep[:cv, cdst:cdst + ci] = True
    R.check_untouched("grad_w", gw, keep, SENT)
    assert (gb[cv:] == SENT).all()
    P, nch = R.wgrad_chunks(rows, wp)
    print(f"wgrad {layer} {grid} (P {P}, {nch} chunks): worst ratio w {ww:.3f} b {wb:.3f}")


# ---- head dgrad -----------------------------------------------------------------------------------------------------------------
_DG_GRIDS = [(1, 3, 5), (2, 7, 9), (3, 13, 10), (4, 30, 40)]                              # rows 35, 198, 540, 5376 (= 42 x 128)


def _h_plane(rows, gen, gpu, plant=None):
    """An activation's bf16 hi plane: relu of random values (half closed), sentinel rows past the end; plant: values written at
    the first interior rows of channel 0.. (zeros, -0, subnormals, a value whose hi rounds to 0)."""
    v = torch.relu(torch.randn(rows, 128, generator=gen))
    hi = v.to(torch.bfloat16)
    if plant is not None:
        for j, (r, vals) in enumerate(plant):
            hi[r, :len(vals)] = torch.tensor(vals).to(torch.bfloat16)
    return torch.cat([hi, torch.full((5, 128), NAN, dtype=torch.bfloat16)]).to(gpu)


def _dgrad_call(gpu, B, h, w, k0, wt, hs, dout=None, gauss=None, acc=None, acc_mode=0, acc_planes=None):
    rows = B * (h + 2) * (w + 2)

    def pl(c):
        return (torch.full((rows + 5, c), SENT, dtype=torch.bfloat16, device=gpu),
                torch.full((rows + 5, c), SENT, dtype=torch.bfloat16, device=gpu))
    dp, d3, d2, d1 = pl(k0), pl(128), pl(128), pl(128)
    a = lib.MagnetHeadDgradArgs(
        dout=dout.data_ptr() if dout is not None else None, k0=k0, wt_hi=wt[0].data_ptr(), wt_lo=wt[1].data_ptr(),
        h3_hi=hs[2].data_ptr(), h2_hi=hs[1].data_ptr(), h1_hi=hs[0].data_ptr(), dout_hi=dp[0].data_ptr(), dout_lo=dp[1].data_ptr(),
        dh3_hi=d3[0].data_ptr(), dh3_lo=d3[1].data_ptr(), dh2_hi=d2[0].data_ptr(), dh2_lo=d2[1].data_ptr(),
        dh1_hi=d1[0].data_ptr(), dh1_lo=d1[1].data_ptr(), acc=acc.data_ptr() if acc is not None else None,
        acc_hi=acc_planes[0].data_ptr() if acc_planes is not None else None,
        acc_lo=acc_planes[1].data_ptr() if acc_planes is not None else None, acc_mode=acc_mode, B=B, h=h, w=w, rows=rows)
    if gauss is not None:
        gg, out, gmm = gauss
        a.grad_gmm, a.gnet_out, a.gmm_in, a.gnet_ld = gg.data_ptr(), out.data_ptr(), gmm.data_ptr(), out.shape[1]
    lib.head_dgrad(a, gpu)
    return dp, d3, d2, d1


def _wt(k0, gen, gpu):
    return tuple(t.to(gpu) for t in split_bf16(torch.randn(128 * k0 + 2 * 16384, generator=gen) * 0.1))


@pytest.mark.parametrize("grid", _DG_GRIDS)
@pytest.mark.parametrize("k0", [160, 128])
def test_head_dgrad_dout_form(hip_lib, gpu, grid, k0):
    B, h, w = grid
    rows = B * (h + 2) * (w + 2)
    gen = _g(rows + k0)
    dout = torch.randn(rows + 5, k0, generator=gen)                                       # live on border rows too
    dout[rows:] = NAN
    dout = dout.to(gpu)
    inner = R.interior_mask(B, h + 2, w + 2, 1).nonzero().flatten()
    plant = [(int(inner[0]), [0.0, -0.0, 2.0 ** -133, -(2.0 ** -133), 2.0 ** -126, 2.0 ** -140, 1.0])]
    hs = [_h_plane(rows, gen, gpu, plant if i == 2 else None) for i in range(3)]
    wt = _wt(k0, gen, gpu)
    outs = _dgrad_call(gpu, B, h, w, k0, wt, hs, dout=dout)
    worst, _, marg = R.check_head_dgrad(f"dgrad k0 {k0} {grid}", B, h, w, k0, wt, hs, outs, dout=dout)
    print(f"head_dgrad k0 {k0} grid {grid} (rows {rows}): worst ratio {worst:.3f}, {marg} marginal")


@pytest.mark.parametrize("grid", _DG_GRIDS)
def test_head_dgrad_gauss_form_with_acc_chain(hip_lib, gpu, grid):
    """G-Net form over three iterations as train.py chains them: acc_mode 1, 2, 2, the split of acc on the last; o1 on both sides
    of 0, exactly 0 and -0."""
    B, h, w = grid
    rows = B * (h + 2) * (w + 2)
    gen = _g(rows)
    wt = _wt(32, gen, gpu)
    acc = torch.full((rows + 5, 128), SENT, device=gpu)
    accp = (torch.full((rows + 5, 128), SENT, dtype=torch.bfloat16, device=gpu),
            torch.full((rows + 5, 128), SENT, dtype=torch.bfloat16, device=gpu))
    inner = R.interior_mask(B, h + 2, w + 2, 1).nonzero().flatten()
    worst = 0.0
    for it in range(3):
        gg = torch.randn(B, 2, h, w, generator=gen).to(gpu)
        gmm = torch.cat([torch.rand(B, 1, h, w, generator=gen) + 1, torch.rand(B, 1, h, w, generator=gen) * 0.5 + 0.05], 1).to(gpu)
        out = torch.full((rows, 16), NAN)
        out[:, :2] = torch.randn(rows, 2, generator=gen) * 2
        out[inner[:4], 1] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
        out = out.to(gpu)
        hs = [_h_plane(rows, gen, gpu) for _ in range(3)]
        mode, last = (1 if it == 0 else 2), it == 2
        old = acc.clone()
        outs = _dgrad_call(gpu, B, h, w, 32, wt, hs, gauss=(gg, out, gmm), acc=acc, acc_mode=mode,
                           acc_planes=accp if last else None)
        wv, s, _ = R.check_head_dgrad(f"gauss {grid} it {it}", B, h, w, 32, wt, hs, outs, gauss=(gg, out, gmm))
        ra, ba = R.acc_ref(s, old[:rows], mode)
        worst = max(worst, wv, R.check(f"gauss {grid} acc it {it}", acc[:rows], ra, ba))
        assert (acc[rows:] == SENT).all()
        if not last:
            assert (accp[0].float() == SENT).all()
    eh, el = split_bf16(acc[:rows])
    R.check_planes_exact("acc planes", accp[0][:rows], accp[1][:rows], eh, el)
    assert (accp[0][rows:].float() == SENT).all()
    print(f"head_dgrad gauss form grid {grid}: worst ratio {worst:.3f} over the acc chain")


# ---- nll --------------------------------------------------------------------------------------------------------------------------
def _nll_backward_into(preds, gt, mask, sums, grad_loss, gamma, out):
    """magnet_nll_loss_backward into a preallocated buffer (NaN-filled by the caller: every element must be written)."""
    l = lib.load()
    I, B, _, H, W = preds.shape
    a = lib.MagnetNllArgs(preds=preds.data_ptr(), gt=gt.data_ptr(), mask=mask.data_ptr(), sums=sums.data_ptr(),
                          grad_loss=grad_loss.data_ptr(), grad_preds=out.data_ptr(), gamma=float(gamma), n_iter=I, B=B, H=H, W=W)
    with torch.cuda.device(preds.device):
        lib._check(l.magnet_nll_loss_backward(ctypes.byref(a), lib._stream(preds)), "magnet_nll_loss_backward")


_NLL = {  # name: (n, B, H, W, gamma)
    "one_pass": (3, 1, 37, 53, 0.8),
    "over_65536": (1, 2, 193, 171, 0.7),                                                # 66 006 pixels, not a multiple of 256
    "n16_4_passes": (16, 3, 257, 341, 0.9),                                             # 262 911 pixels
    "training": (3, 4, 480, 640, 0.8),
}


@pytest.mark.parametrize("case", sorted(_NLL))
def test_nll(hip_lib, gpu, case):
    n, B, H, W, gamma = _NLL[case]
    gen = _g(n * H + W)
    mu = torch.rand(n, B, 1, H, W, generator=gen) * 3 + 1
    sg = torch.rand(n, B, 1, H, W, generator=gen) * 0.5 + 0.02
    edge = torch.tensor([0.0, -1e-3, 9.9e-6, 1e-5, 1.0001e-5, 1.01e-5, -1e-5, 1e-7])   # around sqrt(1e-10f)
    sg.view(-1)[:edge.numel() * 97:97] = edge
    preds = torch.cat([mu, sg], 2).contiguous()
    gt = torch.rand(B, H, W, generator=gen) * 3 + 1
    mask = torch.rand(B, H, W, generator=gen) > 0.25
    if B > 1:
        mask[1] = False                                                                  # one image fully masked
    pg, gtg, mg = preds.to(gpu), gt.to(gpu), mask.to(gpu)
    loss, sums = lib.nll_loss_forward(pg, gtg, mg, gamma)
    r = R.nll_forward_ref(pg, gtg, mg, gamma)
    assert float(sums[0]) == float(r["count"])
    ws = R.check(f"nll {case} sums", sums[1:], *r["sums"])
    wl = R.check(f"nll {case} loss", loss, *r["loss"])
    gl = torch.tensor(2.0 ** 16 * 1.37, device=gpu)                                     # read on the device
    out = torch.full((n * B * 2 * H * W + 11,), NAN, device=gpu)
    _nll_backward_into(pg, gtg, mg, sums, gl, gamma, out)
    ref, bound = R.nll_backward_ref(pg, gtg, mg, sums[0], float(gl), gamma)
    wg = R.check(f"nll {case} grad", out[:ref.numel()].reshape(ref.shape), ref, bound)
    assert torch.isnan(out[ref.numel():]).all()
    print(f"nll {case} ({B * H * W} px, n {n}): worst ratio sums {ws:.3f} loss {wl:.3f} grad {wg:.3f}")


# ---- upsample_depth_backward ------------------------------------------------------------------------------------------------------
_UP = [(1, 1, 1, 1), (2, 1, 7, 3), (1, 5, 1, 2), (3, 13, 9, 16), (2, 17, 23, 3)]          # (B, h, w, n)


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("shape", _UP)
def test_upsample_backward_nchw(hip_lib, gpu, shape, big):
    B, h, w, n = shape
    k = 4
    gen = _g(B * 1000 + h * 10 + w + big)
    depth = (torch.rand(n, B, 2, h, w, generator=gen) + 0.5).to(gpu)
    mask = torch.randn(B, 144, h, w, generator=gen) * 2
    if big:
        mask = torch.where(torch.rand(mask.shape, generator=gen) > 0.5, 80.0, -80.0) + torch.randn(mask.shape, generator=gen)
    mask = mask.to(gpu)
    gup = torch.randn(n, B, 2, k * h, k * w, generator=gen).to(gpu)
    gd, gm = lib.upsample_depth_backward(gup, depth, mask, k)
    r = R.upsample_bwd_ref(gup, depth, mask, k)
    wd = R.check(f"upsample {shape} depth", gd, *r["grad_depth"])
    wm = R.check(f"upsample {shape} mask", gm, *r["grad_mask"])
    print(f"upsample_depth_backward NCHW {shape} logits {'+-80' if big else 'N(0,4)'}: worst ratio depth {wd:.3f} mask {wm:.3f}")


@pytest.mark.parametrize("shape", _UP)
def test_upsample_backward_padded_layout(hip_lib, gpu, shape):
    """The layout train.py passes: logits in the head's (rows, 144) fp32 output, d mask into a zero-bordered (rows, 160) buffer;
    its border rows and channels 144..159 stay as they were."""
    B, h, w, n = shape
    k, ld, mk = 4, 144, 160
    wp, pg = w + 2, (h + 2) * (w + 2)
    rows = B * pg
    gen = _g(B * 77 + h + w)
    mbuf = torch.full((rows, ld), NAN)
    inner = R.interior_mask(B, h + 2, w + 2, 1)
    mbuf[inner] = torch.randn(int(inner.sum()), ld, generator=gen) * 3
    mbuf = mbuf.to(gpu)
    lay = ((wp + 1) * ld, pg * ld, 1, wp * ld, ld)
    glay = ((wp + 1) * mk, pg * mk, 1, wp * mk, mk)
    dmask = torch.full((rows, mk), SENT, device=gpu)
    depth = (torch.rand(n, B, 2, h, w, generator=gen) + 0.5).to(gpu)
    gup = torch.randn(n, B, 2, k * h, k * w, generator=gen).to(gpu)
    gd, _ = lib.upsample_depth_backward(gup, depth, mbuf, k, mask_layout=lay, grad_mask=dmask, grad_mask_layout=glay)
    r = R.upsample_bwd_ref(gup, depth, mbuf, k, mask_layout=lay)
    shp = (B, 144, h, w)
    wd = R.check(f"upsample padded {shape} depth", gd, *r["grad_depth"])
    wm = R.check(f"upsample padded {shape} mask", R.strided(dmask, glay, shp), *r["grad_mask"])
    R.check_untouched("padded grad_mask", dmask, R.addressed(dmask, glay, shp), SENT)
    print(f"upsample_depth_backward padded {shape}: worst ratio depth {wd:.3f} mask {wm:.3f}")
