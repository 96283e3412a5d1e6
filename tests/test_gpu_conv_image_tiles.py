"""Per-image row tiling of the fused 3x3 launches (conv_mfma.hip: ConvParams::tiles_per_img, conv_row_tiles).

The launches with a fused Gaussian update / fused upsampling tile every image on its own, from its first interior image row, when
that takes fewer workgroups than cutting the flattened (B, h+2, w+2) rows from row 0.  Per row the arithmetic does not depend on
the tile, so per-image and flat tiling (MAGNET_TILING_FLAT) must agree bit for bit.  The CPU tests check the tile-count rule
(magnet_conv_row_tiles: host arithmetic, no GPU), the -m gpu tests the launches themselves on the 256-row kernel
(MAGNET_TILING_BM256), w = 14 (wp = 16):

  B x h     per image / flat tiles   form       what it covers
  2 x 40    6 / 6                    flat       3 tiles per image, ragged, tile edges inside image rows: not fewer -> flat
  3 x 33    9 / 7                    flat       per image would be MORE tiles
  5 x 32    10 / 11                  per image  2 exact tiles per image; first and last image at the ends of the buffer
  4 x 31    8 / 9                    per image  ragged last tile, ending on the last row of its image
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

BM = 256
SHAPES = [(2, 40, 14, 6, False), (3, 33, 14, 7, False), (5, 32, 14, 10, True), (4, 31, 14, 8, True)]   # B, h, w, tiles, per image
GUARD = 4096                                      # sentinel floats in front of and behind every output buffer


def _row_tiles(hip_lib, n_img, h, wp, bm):
    per = ctypes.c_int32(-1)
    n = hip_lib.magnet_conv_row_tiles(n_img, h, wp, bm, ctypes.byref(per))
    return n, per.value


def test_tile_rule_on_the_flagship_and_test_shapes(hip_lib):
    assert _row_tiles(hip_lib, 64, 120, 162, 256) == (4864, 76)            # 19 full rounds of 256 workgroups (flat: 4 941)
    assert _row_tiles(hip_lib, 63, 120, 162, 256)[0] == 63 * 76
    assert _row_tiles(hip_lib, 1, 120, 162, 128) == (152, 152)             # one frame, 128-row kernel (flat: 155)
    # last tile of a 120x160 image: rows up to 162 + 76 * 256 - 1 = 19 617 of 19 764 -> inside the bottom border image row
    assert 121 * 162 <= 162 + 76 * 256 - 1 < 122 * 162
    for B, h, w, tiles, by_image in SHAPES:
        n, per = _row_tiles(hip_lib, B, h, w + 2, BM)
        assert n == tiles and (per > 0) == by_image, (B, h, w, n, per)
    assert _row_tiles(hip_lib, 0, 4, 6, 256) == (0, 0) and _row_tiles(hip_lib, 2, 4, 2, 256) == (0, 0)   # bad dimensions


def test_tile_rule_covers_every_interior_row_once_and_keeps_tiles_inside_their_image(hip_lib):
    """All shapes up to 130 x 170 with every B up to 70 at the 256-row tile, every third B at the 128-row tile.  The first row of tile t is the kernel's formula
    (t // per) * (h + 2) * wp + wp + (t % per) * bm; a tile is bm consecutive rows, so the tiles of an image are disjoint and in order.
    The count is never above the flat count; where per-image tiling is chosen it is strictly below it, the tiles of the first and of
    the last image start at the image's first interior image row, cover all its interior rows and end inside the image; and where
    per-image tiling would be fewer tiles and stay inside the image it is not passed over.  (Shapes whose last tile would leave the
    image can never be chosen, whatever B: they are probed at four batch sizes only.)"""
    f = hip_lib.magnet_conv_row_tiles
    per_c = ctypes.c_int32(0)
    ref = ctypes.byref(per_c)
    rec = []
    for bm in (128, 256):
        for h in range(1, 131):
            for w in range(1, 171):
                wp = w + 2
                inside = -(-(h * wp) // bm) * bm <= (h + 1) * wp       # the image's last tile ends inside the image
                Bs = (1, 2, 35, 70) if not inside else range(1, 71) if bm == 256 else (*range(1, 70, 3), 69, 70)
                rec += [(bm, h, wp, B, f(B, h, wp, bm, ref), per_c.value) for B in Bs]
    bm, h, wp, B, n, per = (np.array(c, dtype=np.int64) for c in zip(*rec))
    img = (h + 2) * wp
    flat = -(-(B * img) // bm)
    want_per = -(-(h * wp) // bm)
    inside = want_per * bm <= (h + 1) * wp
    chosen = per > 0
    assert (n[~chosen] == flat[~chosen]).all() and (n <= flat).all()
    assert not (~chosen & inside & (B * want_per < flat)).any()            # the fewer-tiles form is not passed over
    assert chosen.sum() > 100000
    bm, h, wp, B, n, per, img, flat = (a[chosen] for a in (bm, h, wp, B, n, per, img, flat))
    assert (per == want_per[chosen]).all() and (n == B * per).all() and (n < flat).all()
    for i in (np.zeros_like(B), B - 1):                                    # first and last image: tiles i * per .. (i + 1) * per - 1
        t0, t1 = i * per, (i + 1) * per - 1
        first = (t0 // per) * img + wp + (t0 % per) * bm
        last_end = (t1 // per) * img + wp + (t1 % per) * bm + bm
        assert (first == i * img + wp).all()                               # the image's first interior image row
        assert (last_end - first == per * bm).all()                        # per consecutive tiles of bm rows
        assert (last_end >= i * img + (h + 1) * wp).all() and (last_end <= (i + 1) * img).all()   # covers the interior, stays inside


# ---- the launches ------------------------------------------------------------------------------------------------------------------
def _stack(cin, cout_last, seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(cin, 128, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(128, 128, 1), nn.ReLU(inplace=True),
                         nn.Conv2d(128, 128, 1), nn.ReLU(inplace=True), nn.Conv2d(128, cout_last, 1)).eval()


def _guarded(shape, gpu):
    """A NaN-filled output tensor with GUARD NaN floats on either side of it (same allocation)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=gpu)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_untouched(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


_CACHE = {}


def _case(gpu, kind, B, h, w):
    """Inputs, packed weights and the fp32 CPU reference of one case, computed once and shared."""
    key = (kind, B, h, w)
    if key in _CACHE:
        return _CACHE[key]
    from magnet_amd import lib
    from magnet_amd.convnet import ConvStackMFMA
    cin, cout = (320, 2) if kind == "gnet" else (256, 144)
    seq = _stack(cin, cout, seed=41 + cin)
    g = torch.Generator().manual_seed(1000 * B + h)
    x = torch.randn(B, cin, h, w, generator=g)
    depths = [torch.cat([torch.rand(B, 1, h, w, generator=g) * 5 + 0.5, torch.rand(B, 1, h, w, generator=g) * 0.5 + 0.05], dim=1)
              for _ in range(2)]
    with torch.no_grad():
        head = seq(x)                                                  # fp32 torch.nn.functional.conv2d on the CPU
    st = ConvStackMFMA(seq.to(gpu))
    pk = st.packed(gpu)[0]
    rows = B * (h + 2) * (w + 2)
    hi = torch.zeros((rows, cin), dtype=torch.bfloat16, device=gpu); lo = torch.zeros_like(hi)
    lib.pack_split(x.to(gpu), hi, lo, cin, 0)
    _CACHE[key] = dict(st=st, pk=pk, ch=st._chain, hi=hi, lo=lo, rows=rows, cin=cin, head=head, depths=depths)
    return _CACHE[key]


def _launch(c, wp, tiling, **fused):
    from magnet_amd import lib
    pk, ch = c["pk"], c["ch"]
    n = lib.conv_mfma(c["hi"], c["lo"], c["cin"], pk["cin"], pk["w_hi"], pk["w_lo"], pk["bias"], pk["taps"], wp, pk["relu"], c["rows"],
                      tail=(ch["w_hi"], ch["w_lo"], ch["bias"], ch["cout_pad"]), tiling=tiling, **fused)
    torch.cuda.synchronize()
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w,tiles,by_image", SHAPES)
def test_gnet_gaussian_update_per_image_equals_flat(hip_lib, gpu, B, h, w, tiles, by_image):
    """G-Net (cin 320) with the fused Gaussian update, 256-row kernel: grid size by the rule, every interior position written, nothing
    written outside the output, bit-identical to flat tiling, and against fp32 conv2d.
    Bar against fp32: test_gpu_conv.py bounds the head's error by e = 2e-5 max(1, max|head|).  mu' = mu + o0 sigma and
    sigma' = (elu(o1) + 1 + 1e-10) sigma are 1-Lipschitz in (o0, o1) times sigma <= max sigma, so |d out| <= e max(sigma), plus the
    update's own fp32 rounding (a few ulp of max|out|: 1e-6 max|out|)."""
    from magnet_amd import lib
    c = _case(gpu, "gnet", B, h, w)
    gmm = c["depths"][0].to(gpu)
    res = {}
    for name, tiling in (("auto", lib.TILING_BM256), ("flat", lib.TILING_BM256 | lib.TILING_FLAT)):
        buf, out = _guarded(gmm.shape, gpu)
        n = _launch(c, w + 2, tiling, gauss=(gmm, out))
        assert _guards_untouched(buf), f"{name}: write outside the output"
        assert not torch.isnan(out).any(), f"{name}: interior positions left unwritten"
        res[name] = (n, out.clone())
    flat_tiles = -(-c["rows"] // BM)
    assert res["flat"][0] == flat_tiles and res["auto"][0] == tiles and (tiles < flat_tiles) == by_image
    assert torch.equal(res["auto"][1], res["flat"][1]), f"max|d| = {(res['auto'][1] - res['flat'][1]).abs().max().item():.3e}"
    o, g0 = c["head"], c["depths"][0]
    want = torch.stack([g0[:, 0] + o[:, 0] * g0[:, 1], (torch.nn.functional.elu(o[:, 1]) + 1.0 + 1e-10) * g0[:, 1]], dim=1)
    err = (res["auto"][1].cpu() - want).abs().max().item()
    bar = 2e-5 * max(1.0, o.abs().max().item()) * g0[:, 1].max().item() + 1e-6 * want.abs().max().item()
    print(f"[image tiles gnet {B}x{h}x{w}] tiles={res['auto'][0]} flat={flat_tiles} max|d|={err:.3e} bar={bar:.3e}")
    assert err <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("n_pred", [1, 2])
@pytest.mark.parametrize("B,h,w,tiles,by_image", SHAPES)
def test_mask_head_upsampling_per_image_equals_flat(hip_lib, gpu, B, h, w, tiles, by_image, n_pred):
    """Mask head (cin 256) with the fused convex upsampling of n_pred predictions, 256-row kernel: as above.
    Bar against fp32: the logits' error is e = 2e-5 max(1, max|logit|) (test_gpu_conv.py); a softmax weight moves by a factor within
    exp(+-2 e), and the output is a convex combination of depths <= max|depth|, so |d out| <= 2 e max|depth|, plus the 5e-6 that
    test_gpu_conv.py allows the upsampling's own fp32 arithmetic."""
    from magnet_amd import lib
    c = _case(gpu, "mask", B, h, w)
    d = torch.stack(c["depths"][:n_pred]).to(gpu)
    res = {}
    for name, tiling in (("auto", lib.TILING_BM256), ("flat", lib.TILING_BM256 | lib.TILING_FLAT)):
        buf, outs = _guarded((n_pred, B, 2, 4 * h, 4 * w), gpu)
        n = _launch(c, w + 2, tiling, upsample=(d, outs))
        assert _guards_untouched(buf), f"{name}: write outside the output"
        assert not torch.isnan(outs).any(), f"{name}: interior positions left unwritten"
        res[name] = (n, outs.clone())
    flat_tiles = -(-c["rows"] // BM)
    assert res["flat"][0] == flat_tiles and res["auto"][0] == tiles and (tiles < flat_tiles) == by_image
    assert torch.equal(res["auto"][1], res["flat"][1]), f"max|d| = {(res['auto'][1] - res['flat'][1]).abs().max().item():.3e}"
    m = c["head"]
    mk = torch.softmax(m.view(B, 1, 9, 4, 4, h, w), dim=2)
    got = res["auto"][1].cpu()
    bar = 2 * 2e-5 * max(1.0, m.abs().max().item()) * d.abs().max().item() + 5e-6
    for i in range(n_pred):
        up = torch.nn.functional.unfold(c["depths"][i], [3, 3], padding=1).view(B, 2, 9, 1, 1, h, w)
        want = torch.sum(mk * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 4 * h, 4 * w)
        err = (got[i] - want).abs().max().item()
        print(f"[image tiles mask {B}x{h}x{w} pred {i}] tiles={res['auto'][0]} flat={flat_tiles} max|d|={err:.3e} bar={bar:.3e}")
        assert err <= bar
