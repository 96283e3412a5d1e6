"""magnet_conv_mfma_nchw: the fused 3x3 launches with x_d3 read in place as NCHW fp32 and split to (hi, lo) bf16 in LDS.

The kernel writes into the window slot of the K loop the bytes the plane DMA would have put there, so every case compares the new
entry point BIT FOR BIT (torch.equal on int32 views) with lib.pack_split + magnet_conv_mfma_ex on the same 256-row kernel
(MAGNET_TILING_BM256; every case is below 65 536 rows).  Forms: G-Net (cin 320 = 64 plane channels + 256 from src, fused Gaussian
update) and mask head (cin 256, src_c0 = 0, no planes at all, fused upsampling of 1 and 2 predictions).

  B x h x w     wp    tiles / image   what it covers
  5 x 32 x 14   16    2               a wave's 32-row run crosses two image-row ends; first / last image at the ends of the buffer
  4 x 31 x 14   16    2               ragged: the last tile ends on the image's last border row; h w = 434 pixels, so a channel's base
                                      is only 8-byte aligned and the 16-byte rounding of a run start differs between channels
  2 x 15 x 32   34    2               two tiles per image, wp no power of two
  2 x 11 x 160  162   7               the flagship pitch: a tile's halo reaches the image row above and below

What must not be read holds NaN: the x_d3 channels of the plane buffer, and 64 KB in front of and behind src (same allocation).
Outputs are NaN-filled inside guards: every interior position must be written and nothing else."""
import numpy as np
import pytest
import torch
import torch.nn as nn

SHAPES = [(5, 32, 14), (4, 31, 14), (2, 15, 32), (2, 11, 160)]
GUARD = 16384                                     # floats: 64 KB on either side of src and of every output
DP = 64                                           # plane channels of the G-Net form (the cost channels)


def _stack(cin, cout_last, seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(cin, 128, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(128, 128, 1), nn.ReLU(inplace=True),
                         nn.Conv2d(128, 128, 1), nn.ReLU(inplace=True), nn.Conv2d(128, cout_last, 1)).eval()


def _guarded(shape, gpu, fill=None):
    """A tensor inside a NaN-filled allocation with GUARD NaN floats on either side; itself NaN, or a copy of `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=gpu)
    t = buf[GUARD:GUARD + n].view(shape)
    if fill is not None:
        t.copy_(fill)
    return buf, t


def _guards_untouched(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


_WEIGHTS = {}


def _weights(gpu, kind):
    if kind not in _WEIGHTS:
        from magnet_amd.convnet import ConvStackMFMA
        cin, cout = (DP + 256, 2) if kind == "gnet" else (256, 144)
        st = ConvStackMFMA(_stack(cin, cout, seed=7 + cin).to(gpu))
        _WEIGHTS[kind] = (st, st.packed(gpu)[0], st._chain)
    return _WEIGHTS[kind]


def _inputs(B, h, w, planted=False):
    g = torch.Generator().manual_seed(100 * B + h + w)
    x = torch.randn(B, 256, h, w, generator=g)
    cost = torch.randn(B, DP, h, w, generator=g)
    depths = torch.stack([torch.cat([torch.rand(B, 1, h, w, generator=g) * 5 + 0.5, torch.rand(B, 1, h, w, generator=g) * 0.5 + 0.05], dim=1)
                          for _ in range(2)])
    if planted:
        vals = [float("inf"), float("-inf"), float("nan"), -0.0, 1e-40, -3e-39, 3.4e38, -3.4e38]
        places = [(0, 0, 0), (B - 1, h - 1, w - 1), (0, h // 2, 0), (B - 1, h // 2, w - 1), (0, 1, w - 1), (B - 1, h - 2, 0)]   # b, y, x
        i = 0
        for c in (0, 255):
            for b, y, xx in places:
                x[b, c, y, xx] = vals[i % len(vals)]
                i += 1
        x[0, 17, 0, 1] = vals[2]; x[B - 1, 130, h - 1, w - 2] = vals[0]
    return x, cost, depths


def _run_pair(gpu, kind, B, h, w, n_pred=1, planted=False):
    """(tiles, out, guard buffer) of the packed reference launch and of the in-place launch."""
    from magnet_amd import lib
    st, pk, ch = _weights(gpu, kind)
    x, cost, depths = _inputs(B, h, w, planted)
    wp, rows = w + 2, B * (h + 2) * (w + 2)
    cin = pk["cin"]
    sbuf, src = _guarded(x.shape, gpu, x)
    hi = torch.zeros((rows, cin), dtype=torch.bfloat16, device=gpu); lo = torch.zeros_like(hi)
    if kind == "gnet":
        lib.pack_split(cost.to(gpu), hi, lo, cin, 0)
        hi_n, lo_n = hi.clone(), lo.clone()
        hi_n[:, DP:] = float("nan"); lo_n[:, DP:] = float("nan")       # the x_d3 channels of the planes must not be read
        lib.pack_split(src, hi, lo, cin, DP)
        planes_n, c0 = (hi_n, lo_n), DP
    else:
        lib.pack_split(src, hi, lo, cin, 0)
        planes_n, c0 = (None, None), 0
    res = []
    for planes, extra in (((hi, lo), {}), (planes_n, dict(src_nchw=(src, c0)))):
        if kind == "gnet":
            buf, out = _guarded((B, 2, h, w), gpu)
            fused = dict(gauss=(depths[0].to(gpu), out))
        else:
            buf, out = _guarded((n_pred, B, 2, 4 * h, 4 * w), gpu)
            fused = dict(upsample=(depths[:n_pred].to(gpu), out))
        n = lib.conv_mfma(planes[0], planes[1], cin, cin, pk["w_hi"], pk["w_lo"], pk["bias"], pk["taps"], wp, pk["relu"], rows,
                          tail=(ch["w_hi"], ch["w_lo"], ch["bias"], ch["cout_pad"]), tiling=lib.TILING_BM256, **fused, **extra)
        torch.cuda.synchronize()
        res.append((n, out, buf))
    assert _guards_untouched(sbuf) and torch.equal(src.cpu().view(torch.int32), x.view(torch.int32)), "src or its guards were written"
    return res


def _check(res, B, h, w, planted=False):
    from magnet_amd import lib
    tiles, per = lib.conv_row_tiles(B, h, w + 2, 256)
    assert per > 0 and tiles == B * per and h * (w + 2) <= per * 256 <= (h + 1) * (w + 2)
    (n_ref, ref, rbuf), (n_new, new, nbuf) = res
    assert n_ref == tiles and n_new == tiles
    assert _guards_untouched(rbuf) and _guards_untouched(nbuf), "write outside the output"
    if not planted:
        assert not torch.isnan(ref).any() and not torch.isnan(new).any(), "interior positions left unwritten"
    d = (new.view(torch.int32) != ref.view(torch.int32))
    assert not d.any(), f"{int(d.sum())} of {d.numel()} outputs differ in their bits"


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_gnet_in_place_equals_packed(hip_lib, gpu, B, h, w):
    _check(_run_pair(gpu, "gnet", B, h, w), B, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("n_pred", [1, 2])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_mask_head_in_place_equals_packed(hip_lib, gpu, B, h, w, n_pred):
    _check(_run_pair(gpu, "mask", B, h, w, n_pred=n_pred), B, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gnet", "mask"])
@pytest.mark.parametrize("B,h,w", [(4, 31, 14), (2, 15, 32)])
def test_planted_special_values_equal_packed(hip_lib, gpu, B, h, w, kind):
    """+-Inf, NaN, -0, fp32 denormals and +-3.4e38 at the first and last pixel of an image, beside either border column, in channel 0
    and channel 255: the split in LDS is the pack's (hi = bf16(x), lo = bf16(x - hi)), so the outputs agree in their bits, NaNs included."""
    res = _run_pair(gpu, kind, B, h, w, n_pred=2, planted=True)
    _check(res, B, h, w, planted=True)
    assert torch.isnan(res[0][1]).any()                                # the planted values did reach outputs
