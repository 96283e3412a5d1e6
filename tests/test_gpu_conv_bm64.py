"""The 64-row tile form of the 3x3 launches (MAGNET_TILING_BM64; csrc/conv_mfma.hip: conv_mfma_kernel<8,2,64,1,T,256,false,2>, T = 0, 1,
8, 9), the latency-mode instances that ConvStackMFMA takes by itself when the 128-row tiling under-fills the chip.

  pointwise      every instance against the fp64 restatement and the derived bounds of tests/conv_fwd_ref.py, on the shape, inputs,
                 sentinel bands and checks of tests/test_gpu_conv_fwd.py (helpers imported, not restated): 2 x 9 x 13, 330 rows =
                 6 tiles of 64 rows, the last with 10 rows.
  bit-identity   the fused Gaussian update and the fused upsampling, default instance against TILING_BM64, torch.equal on everything a
                 launch writes; grids (w + 2 = wp; the tile counts are conv_row_tiles' at bm = 64, asserted):
                   B x h x w     wp  64-row tiles   form        what it reaches
                   2 x 8 x 14    16  4 (flat 5)     per image   2 exact tiles per image
                   4 x 7 x 14    16  8 (flat 9)     per image   each image's last tile ends exactly at the image's last row
                   3 x 9 x 14    16  9              flat        per image would leave the image
                   2 x 10 x 13   15  6              flat        odd pitch, tile edges inside image rows
  model          a stand-in MAGNET at one 24 x 32 frame: small_tiles False against "auto" and True, every returned tensor torch.equal,
                 and last_tiles shows which instance ran.  "auto" is run with the rule's candidate limit of 256 tiles (the shipped
                 limit is the measured one, profiles/latency/NOTES.md: 0, "auto" = the 128-row launches; that is asserted too).
  rejections     flag combinations without an instance raise MAGNET_E_DIM before anything is launched.
"""
import pytest
import torch

from magnet_amd import synth
from tests import conv_fwd_ref as C
from tests.test_gpu_conv_fwd import EXTRA, _assert_untouched, _case, _guarded, _is_sentinel, _launch, _ref, _tail_pack
from tests.test_gpu_conv_image_tiles import _case as _stack_case
from tests.test_gpu_conv_image_tiles import _guarded as _guarded_f32
from tests.test_gpu_conv_image_tiles import _guards_untouched
from tests.test_gpu_conv_image_tiles import _launch as _stack_launch

BM = 64
TILES_330 = 6                                     # 330 rows: five whole 64-row tiles and one of 10 rows


# ---- pointwise against fp64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tail_cout", [16, 128, 144])
@pytest.mark.parametrize("cin,addend", [(64, False), (32, True)], ids=["t9-cin64", "addend-cin32"])
def test_fused_tail_bm64(hip_lib, gpu, request, cin, addend, tail_cout):
    """<8,2,64,1,T,256,false,2>, T = 1, 8, 9: 3x3 first layer (bias, ReLU, with and without the hoisted layer's addend) + the three fused
    1x1 layers; test_fused_tail's inputs, reference, bound and sentinel bands."""
    from magnet_amd import lib
    name = request.node.callspec.id
    c = _case(gpu, 2, 9, 13, 1, cin, 128, 9)
    assert c["rows"] == 330
    t = _tail_pack(gpu, tail_cout)
    a0, b0 = _ref(c, relu=True, addend=addend)
    ref, bound = C.tail_ref(a0, C.split_bound(a0, b0), t["w64"], t["bias"], tail_cout)
    buf, body = _guarded((c["rows"] + EXTRA, tail_cout), gpu)
    tiles = _launch(c, dict(out_f32=body), relu=True, addend=addend, tiling=lib.TILING_BM64, tail=(t["wh"], t["wl"], t["bias"], tail_cout))
    assert tiles == TILES_330, f"{name}: {tiles} tiles: not the 64-row instance"
    _assert_untouched(name, buf, body, 0, tail_cout, c["rows"])
    inner = c["inner"]
    worst = C.check(name, body[:c["rows"]][inner], ref[inner], bound[inner])
    print(f"[conv bm64 tail {name}] tiles={tiles} worst ratio {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(relu=True), dict(border=True, relu=True), dict(res=True, relu=True), dict(addend=True)],
                         ids=["relu", "border", "residual", "addend"])
def test_plain_bm64(hip_lib, gpu, request, kw):
    """<8,2,64,1,0,256,false,2>, fp32 output: the plain epilogue and its border / residual / addend features (the x_d3 part of G-Net's
    hoisted first layer is the fp32 form without bias activation)."""
    from magnet_amd import lib
    name = request.node.callspec.id
    c = _case(gpu, 2, 9, 13, 1, 64, 128, 9)
    ref, bound = _ref(c, **{k: v for k, v in kw.items() if k != "border"})
    written = c["inner"]
    if kw.get("border"):
        ref, bound, written = C.border_and_repad(ref, bound, c["N"], c["hp"], c["wp"], c["pad"])
    buf, body = _guarded((c["rows"] + EXTRA, 128), gpu)
    tiles = _launch(c, dict(out_f32=body), tiling=lib.TILING_BM64, **kw)
    assert tiles == TILES_330, f"{name}: {tiles} tiles: not the 64-row instance"
    _assert_untouched(name, buf, body, 0, 128, c["rows"])
    worst = C.check(name, body[:c["rows"]][written], ref[written], bound[written])
    print(f"[conv bm64 plain {name}] tiles={tiles} worst ratio {worst:.3f}")


@pytest.mark.gpu
def test_output_modes_bm64(hip_lib, gpu):
    """fp32, split planes and the single bf16 plane (border zeroing, ReLU, residual), as test_output_modes: the fp32 output against the
    bound, the planes its split_bf16 and the bf16 plane its round-to-nearest-even, bit for bit; border zeros are +0."""
    from magnet_amd import lib
    from magnet_amd.convnet import split_bf16
    c = _case(gpu, 2, 9, 13, 1, 64, 128, 9)
    kw = dict(relu=True, res=True, border=True, tiling=lib.TILING_BM64)
    rows = c["rows"]
    ref, bound = _ref(c, relu=True, res=True)
    ref, bound, _ = C.border_and_repad(ref, bound, c["N"], c["hp"], c["wp"], c["pad"])
    bufs = {mode: _guarded((rows + EXTRA, 128), gpu, dtype)
            for mode, dtype in (("f32", torch.float32), ("hi", torch.bfloat16), ("lo", torch.bfloat16), ("bf16", torch.bfloat16))}
    assert _launch(c, dict(out_f32=bufs["f32"][1]), **kw) == TILES_330
    assert _launch(c, dict(out_hi=bufs["hi"][1], out_lo=bufs["lo"][1]), **kw) == TILES_330
    assert _launch(c, dict(out_bf16=bufs["bf16"][1]), **kw) == TILES_330
    for mode, (buf, body) in bufs.items():
        _assert_untouched(f"bm64 {mode}", buf, body, 0, 128, rows)
    f32 = bufs["f32"][1][:rows]
    worst = C.check("bm64 fp32", f32, ref, bound)
    eh, el = split_bf16(f32)
    C.check_planes_exact("bm64 split planes", bufs["hi"][1][:rows], bufs["lo"][1][:rows], eh, el)
    assert torch.equal(bufs["bf16"][1][:rows].view(torch.int16), f32.to(torch.bfloat16).view(torch.int16)), "bf16 plane is not RNE(fp32)"
    edge = ~c["inner"]
    assert bool((f32[edge].view(torch.int32) == 0).all()), "fp32 border outputs are not +0"
    for mode in ("hi", "lo", "bf16"):
        assert bool((bufs[mode][1][:rows][edge].view(torch.int16) == 0).all()), f"{mode} plane: border outputs are not +0"
    print(f"[conv bm64 output modes] worst ratio (fp32) {worst:.3f}; planes and bf16 plane bit-exact")


@pytest.mark.gpu
def test_plain_bm64_equals_default_bit_for_bit(hip_lib, gpu):
    """The K order of an output element does not depend on the tile: the 64-row and the 128-row plain instances agree to the bit on
    every interior row (the plain form leaves border rows unspecified)."""
    from magnet_amd import lib
    c = _case(gpu, 2, 9, 13, 1, 64, 128, 9)
    outs = []
    for tiling in (0, lib.TILING_BM64):
        _, body = _guarded((c["rows"] + EXTRA, 128), gpu)
        _launch(c, dict(out_f32=body), relu=True, tiling=tiling)
        outs.append(body[:c["rows"]][c["inner"]])
    assert torch.equal(outs[0], outs[1])


# ---- bit-identity with the default instance: the fused Gaussian update and the fused upsampling ---------------------------------------
#          B  h   w   64-row tiles  per image
SHAPES = [(2, 8,  14, 4,            True),
          (4, 7,  14, 8,            True),
          (3, 9,  14, 9,            False),
          (2, 10, 13, 6,            False)]


def _three_ways(c, w, by_image, tiles, make_out, **fused):
    """The launch with tiling 0, BM64 and (per-image shapes) FLAT | BM64: outputs of the first two, after the assertions on all."""
    from magnet_amd import lib
    flat_tiles = -(-c["rows"] // BM)
    assert (tiles < flat_tiles) == by_image
    res = {}
    for name, tiling in (("default", 0), ("bm64", lib.TILING_BM64), ("flat", lib.TILING_FLAT | lib.TILING_BM64)):
        buf, out = make_out()
        n = _stack_launch(c, w + 2, tiling, **{k: (v, out) for k, v in fused.items()})
        assert _guards_untouched(buf), f"{name}: write outside the output"
        assert not torch.isnan(out).any(), f"{name}: interior positions left unwritten"
        res[name] = (n, out.clone())
    assert res["bm64"][0] == tiles and res["flat"][0] == flat_tiles, (res["bm64"][0], res["flat"][0])
    assert torch.equal(res["bm64"][1], res["default"][1]), f"max|d| = {(res['bm64'][1] - res['default'][1]).abs().max().item():.3e}"
    assert torch.equal(res["flat"][1], res["bm64"][1]), "flat and per-image 64-row tilings differ"
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w,tiles,by_image", SHAPES)
def test_gnet_gaussian_update_bm64_equals_default(hip_lib, gpu, B, h, w, tiles, by_image):
    """G-Net (cin 320) with the fused Gaussian update: <8,2,64,1,1,...> writes what <8,2,128,1,1,...> writes, bit for bit."""
    c = _stack_case(gpu, "gnet", B, h, w)
    gmm = c["depths"][0].to(gpu)
    res = _three_ways(c, w, by_image, tiles, lambda: _guarded_f32(gmm.shape, gpu), gauss=gmm)
    print(f"[conv bm64 gnet {B}x{h}x{w}] tiles default={res['default'][0]} bm64={res['bm64'][0]} flat={res['flat'][0]}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_pred", [1, 3])
@pytest.mark.parametrize("B,h,w,tiles,by_image", SHAPES)
def test_mask_head_upsampling_bm64_equals_default(hip_lib, gpu, B, h, w, tiles, by_image, n_pred):
    """Mask head (cin 256) with the fused convex upsampling of n_pred predictions: one 64-row pass through the LDS stage against the
    128-row instance's, bit for bit."""
    c = _stack_case(gpu, "mask", B, h, w)
    d = torch.stack([c["depths"][i % 2] * (1.0 + 0.25 * (i // 2)) for i in range(n_pred)]).to(gpu)
    res = _three_ways(c, w, by_image, tiles, lambda: _guarded_f32((n_pred, B, 2, 4 * h, 4 * w), gpu), upsample=d)
    print(f"[conv bm64 mask {B}x{h}x{w} n_pred={n_pred}] tiles default={res['default'][0]} bm64={res['bm64'][0]} flat={res['flat'][0]}")


# ---- the model takes it by itself ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D,iters", [(5, 3), (64, 1)], ids=["D5-I3-hoisted", "D64-I1"])
def test_model_auto_equals_parent_launches(hip_lib, gpu, monkeypatch, D, iters):
    """One 24 x 32 frame (884 rows: 7 tiles of 128 rows) through MAGNET.forward with stand-in backbones: small_tiles False (the 128-row
    launches) against "auto" under a limit of 256 tiles and against True, every returned tensor bit-identical; last_tiles names the
    instance.  D = 5, I = 3 runs the hoisted invariant launch and three addend launches, D = 64, I = 1 the single fused launch.
    Under the shipped limit "auto" launches what use_small_tiles says for 7 tiles."""
    from magnet_amd import convnet
    from magnet_amd.convnet import ConvStackMFMA
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import StubDNet, StubFNet, make_args, seeded_magnet_weights
    wl = synth.Workload("bm64", "scannet", 24, 32, V=2, D=D, F=16)
    inp = synth.make_inputs(wl, B=1, seed=3)
    m = MAGNET(make_args(D=D, iters=iters, dpv_h=24, dpv_w=32), d_net=StubDNet(1), f_net=StubFNet(2, fdim=16))
    seeded_magnet_weights(m, 3)
    m = m.to(gpu).eval()
    g = torch.Generator().manual_seed(0)
    ref_img, nb_img = torch.rand(1, 3, 96, 128, generator=g).to(gpu), torch.rand(2, 3, 96, 128, generator=g).to(gpu)
    assert ConvStackMFMA.small_tiles == "auto"
    outs, tiles = {}, {}
    shipped_says = convnet.use_small_tiles(1, 24, 34)
    for mode, limit in ((False, None), ("auto", 256), (True, None), ("shipped", None)):
        monkeypatch.setattr(ConvStackMFMA, "small_tiles", "auto" if mode == "shipped" else mode)
        monkeypatch.setattr(ConvStackMFMA, "record_tiles", True)       # last_tiles: the tile counts the library reports
        if limit is not None:
            monkeypatch.setattr(convnet, "SMALL_TILE_LIMIT", limit)
        with torch.no_grad():
            preds = m(ref_img, nb_img, inp["nghbr_poses"].to(gpu), inp["is_valid"], inp["cam_intrins"], mode="test")
        torch.cuda.synchronize()
        outs[mode] = [p.clone() for p in preds]
        g_stack, m_stack = m._stacks
        tiles[mode] = (list(g_stack.last_invariant_tiles) if iters >= 2 else [], list(g_stack.last_tiles), list(m_stack.last_tiles))
        monkeypatch.undo()
    for mode in ("auto", True, "shipped"):
        assert len(outs[False]) == len(outs[mode]) == iters
        for a, b in zip(outs[False], outs[mode]):
            assert a.shape == (1, 2, 96, 128) and torch.isfinite(a).all() and torch.equal(a, b)
    rows = 26 * 34
    n128, n64 = -(-rows // 128), -(-rows // 64)
    per64 = -(-24 * 34 // 64)                     # fused update / upsampling: per image when fewer tiles that end inside the image
    fused64 = per64 if per64 < n64 and per64 * 64 <= 25 * 34 else n64
    per128 = -(-24 * 34 // 128)
    fused128 = per128 if per128 < n128 and per128 * 128 <= 25 * 34 else n128
    hoisted = iters >= 2
    assert tiles[False] == ([(128, n128)] if hoisted else [], [(128, fused128)], [(128, fused128)])
    assert tiles["auto"] == tiles[True] == ([(64, n64)] if hoisted else [], [(64, fused64)], [(64, fused64)])
    assert tiles["shipped"] == (tiles[True] if shipped_says else tiles[False])
    if not shipped_says:                          # nothing to decide and nothing asked for: the plain launches, no record
        with torch.no_grad():
            m(ref_img, nb_img, inp["nghbr_poses"].to(gpu), inp["is_valid"], inp["cam_intrins"], mode="test")
        assert list(m._stacks[0].last_tiles) == [] and list(m._stacks[1].last_tiles) == []


@pytest.mark.gpu
@pytest.mark.parametrize("record", [False, True], ids=["plain-entry", "recorded"])
def test_model_auto_with_a_positive_limit_that_says_no(hip_lib, gpu, monkeypatch, record):
    """"auto" with a limit of 5 tiles at a launch of 7: there is something to decide, the rule says no, and (record_tiles off) nothing is
    reported.  The hoisted forward (D = 5, I = 3: run_invariant and three addend launches) runs, equals small_tiles = False bit for
    bit, records nothing without record_tiles and the 128-row tiles with it."""
    from magnet_amd import convnet
    from magnet_amd.convnet import ConvStackMFMA
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import StubDNet, StubFNet, make_args, seeded_magnet_weights
    wl = synth.Workload("bm64-no", "scannet", 24, 32, V=2, D=5, F=16)
    inp = synth.make_inputs(wl, B=1, seed=3)
    m = MAGNET(make_args(D=5, iters=3, dpv_h=24, dpv_w=32), d_net=StubDNet(1), f_net=StubFNet(2, fdim=16))
    seeded_magnet_weights(m, 3)
    m = m.to(gpu).eval()
    g = torch.Generator().manual_seed(0)
    ref_img, nb_img = torch.rand(1, 3, 96, 128, generator=g).to(gpu), torch.rand(2, 3, 96, 128, generator=g).to(gpu)
    outs = {}
    for mode in (False, "auto"):
        monkeypatch.setattr(ConvStackMFMA, "small_tiles", mode)
        monkeypatch.setattr(ConvStackMFMA, "record_tiles", record)
        monkeypatch.setattr(convnet, "SMALL_TILE_LIMIT", 5)
        assert not convnet.use_small_tiles(1, 24, 34) and not convnet.use_small_tiles(1, 24, 34, by_image=False)
        with torch.no_grad():
            outs[mode] = [p.clone() for p in m(ref_img, nb_img, inp["nghbr_poses"].to(gpu), inp["is_valid"], inp["cam_intrins"], mode="test")]
        torch.cuda.synchronize()
        g_stack, m_stack = m._stacks
        want = [(128, 7)] if record else []
        assert list(g_stack.last_invariant_tiles) == want and list(g_stack.last_tiles) == want and list(m_stack.last_tiles) == want
        monkeypatch.undo()
    assert len(outs[False]) == len(outs["auto"]) == 3
    for a, b in zip(outs[False], outs["auto"]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bm64_without_an_instance_is_rejected(hip_lib, gpu):
    """BM64 | BM256, BM64 on a 1x1 launch and BM64 at cout_pad 64: MAGNET_E_DIM, and the output buffer keeps every sentinel."""
    from magnet_amd import lib
    t = _tail_pack(gpu, 16)
    tail = (t["wh"], t["wl"], t["bias"], 16)
    cases = [("bm64|bm256", _case(gpu, 2, 9, 13, 1, 64, 128, 9), lib.TILING_BM64 | lib.TILING_BM256, tail, 16),
             ("taps 1 fused", _case(gpu, 2, 9, 13, 1, 64, 128, 1), lib.TILING_BM64, tail, 16),
             ("taps 1 plain", _case(gpu, 2, 9, 13, 1, 64, 128, 1), lib.TILING_BM64, None, 128),
             ("cout_pad 64", _case(gpu, 2, 9, 13, 1, 64, 64, 9), lib.TILING_BM64, None, 64)]
    for name, c, tiling, tl, cout in cases:
        buf, body = _guarded((c["rows"] + EXTRA, cout), gpu)
        with pytest.raises(lib.MagnetError, match="MAGNET_TILING_BM64") as ei:
            _launch(c, dict(out_f32=body), relu=True, tiling=tiling, tail=tl)
        assert ei.value.code == lib.E_DIM, name
        torch.cuda.synchronize()
        assert bool(_is_sentinel(buf).all()), f"{name}: the rejected launch wrote"
