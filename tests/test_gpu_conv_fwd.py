"""Every forward conv_mfma instance, one direct launch each, against the fp64 restatement of tests/conv_fwd_ref.py, pointwise.

Each test makes ONE lib.conv_mfma / lib.pack_split call on planes split with convnet.split_bf16 and weights packed
with planes.pack_taps, and compares it with the reference of exactly the planes the kernel received through `check` (|got - ref| <=
bound at every element; the bound is derived in conv_fwd_ref.py, not measured).  Outputs live inside one allocation with NaN guard
bands on both sides; rows at or past `rows`, channels outside a written slice and (under repad) the target grid's border must keep
their sentinel bit for bit.  Biases are random and non-zero in every padded channel, and every padded output channel is compared.
Inputs are heavy-tailed (cubes of normals) and the fused tails' weights non-negative: single terms dominate some outputs and the 1x1
layers do not cancel, which is where the bounds are sharp (tests/test_conv_fwd_ref.py plants the defects these inputs expose).

Dispatch of launch_conv_mfma at variant == 0 (csrc/conv_mfma.hip), first match wins; the ids of the parametrised cases name the
instance <NF, WN, BM, TAIL, NT, PP, WIN> they reach (NF 16-channel fragments per workgroup, WN waves along N, BM rows per tile, NT
threads, PP the 8-wave ping-pong loop, WIN 2 = register row window, 1 = 2-slot LDS window, 0 = flat loop).  The tile count the
library reports (rows / BM rounded up) is asserted, which tells the 128-row from the 256-row instances.

  fused tail (tail_w_hi; cout_pad must be 128; T = tail_cout / 16 = 1, 8, 9)
    taps 9 and (rows >= 65536 or TILING_BM256) and no addend                <8,2,256,T,512,PP,2>    test_fused_tail[bm256-*]
    taps 9 (so also: addend under TILING_BM256, the hoisted first layer)    <8,2,128,T,256,-,2>     test_fused_tail[t9-*], [addend*-*]
    taps 4                                                                  <8,2,128,T,256,-,1>     test_fused_tail[t4-*]
    taps 1                                                                  <8,2,128,T,256,-,0>     test_fused_tail[t1-*]
  plain
    cout_pad 128, taps 9, fp32 out, rows >= 65536, no residual, no border   <8,2,256,0,512,PP,2>    test_plain_8wave
    cout_pad % 128 == 0, taps 9                                             <8,2,128,0,256,-,2>     nf8_win2-*
    cout_pad % 128 == 0, taps 4                                             <8,2,128,0,256,-,1>     nf8_win1-*
    cout_pad % 128 == 0 (taps 1)                                            <8,2,128,0,256,-,0>     nf8_flat-*
    cout_pad 144 (any taps)                                                 <9,1,128,0,256,-,0>     nf9_flat-*
    cout_pad 16 (any taps)                                                  <1,1,128,0,256,-,0>     nf1_flat-*
    cout_pad 32 / 64, taps 9                                                <2|4,1,128,0,256,-,2>   nf2_win2-*, nf4_win2-*
    cout_pad 32 / 64 (taps 4, 1)                                            <2|4,1,128,0,256,-,0>   nf2_flat-*, nf4_flat-*
  launch_pack_split (csrc/pack.hip): h*w % 4 == 0, C % 8 == 0, in_img_stride % 4 == 0, 16-byte aligned input ->
    pack_nchw_kernel<PackSplit, 128>, else pack_nchw_kernel<PackSplit, 64>                          test_pack_split

Not repeated here, because existing tests tie them bit for bit to launches that ARE checked here:
  the fused Gaussian update and the fused upsampling     test_gpu_conv.py::test_gnet_with_fused_gaussian_update_equals_the_two_launch_form,
                                                         ::test_mask_head_with_fused_upsampling_equals_the_two_launch_form (= the plain
                                                         tail + the stand-alone kernel), and test_gpu_conv_image_tiles.py (per-image ==
                                                         flat tiling).  The stand-alone kernels (magnet_gaussian_update_cl,
                                                         magnet_upsample_depth_cl / _cl_n) are the anchor of that chain: they are
                                                         checked against fp64 with derived pointwise bounds, at block-edge shapes
                                                         and edge inputs, in tests/test_gpu_elementwise_fwd.py (restatements and
                                                         bounds: tests/elementwise_fwd_ref.py)
"""
import pytest
import torch

from tests import conv_fwd_ref as C
from tests.conv_fwd_ref import GUARD, guarded as _guarded  # noqa: F401  (other test modules import them from here)

EXTRA = 40                                        # sentinel rows behind the last row a launch may write
NAN_BITS = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0}
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _heavy(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_g(seed)) ** 3 * scale


def _is_sentinel(t):
    """Elementwise: still the NaN the buffer was filled with, bit for bit."""
    return t.contiguous().view(INT_OF[t.dtype]) == NAN_BITS[t.dtype]


def _assert_untouched(name, buf, body, c0, c1, rows_written):
    """Guards, the rows from rows_written on, and the channels outside [c0, c1) of every row keep the sentinel."""
    assert bool(_is_sentinel(buf[:GUARD]).all() and _is_sentinel(buf[-GUARD:]).all()), f"{name}: write outside the output buffer"
    assert bool(_is_sentinel(body[rows_written:]).all()), f"{name}: a row at or past `rows` was written"
    assert bool(_is_sentinel(body[:, :c0]).all() and _is_sentinel(body[:, c1:]).all()), f"{name}: a channel outside the slice was written"


_CACHE = {}


def _case(gpu, N, h, w, pad, cin, cout, taps, dil=1, in_wide=False, seed=0):
    """Planes, pack, bias, residual, addend and the fp64 pre-activation pieces of one shape, built once and shared, never modified."""
    key = (N, h, w, pad, cin, cout, taps, dil, in_wide, seed)
    if key in _CACHE:
        return _CACHE[key]
    from magnet_amd.convnet import split_bf16
    from magnet_amd.planes import pack_taps
    hp, wp = h + 2 * pad, w + 2 * pad
    rows = N * hp * wp
    in_ld, c0 = (cin + 24, 16) if in_wide else (cin, 0)
    xb = torch.randn((N, hp, wp, in_ld), generator=_g(10 + seed))      # the channels around the slice hold data, not zeros
    xb[..., c0:c0 + cin] = 0
    xb[:, pad:pad + h, pad:pad + w, c0:c0 + cin] = _heavy((N, h, w, cin), 11 + seed)
    hi, lo = split_bf16(xb.reshape(rows, in_ld).to(gpu))
    k = {9: 3, 4: 2, 1: 1}[taps]
    wh, wl = pack_taps(_heavy((cout, cin, k, k), 12 + seed, (taps * cin) ** -0.5).to(gpu))
    bias = (torch.randn(cout, generator=_g(13 + seed)) * 0.5).to(gpu)
    assert bool((bias != 0).all())
    rh, rl = split_bf16(_heavy((rows, cout + 8), 14 + seed).to(gpu))
    addend = _heavy((rows, cout + 8), 15 + seed).to(gpu)
    c = dict(N=N, h=h, w=w, pad=pad, hp=hp, wp=wp, rows=rows, cin=cin, cout=cout, taps=taps, dil=dil, in_ld=in_ld,
             hi=hi[:, c0:c0 + cin], lo=lo[:, c0:c0 + cin], wh=wh, wl=wl, bias=bias, res=(rh, rl, cout + 8), addend=addend,
             inner=C.interior(N, hp, wp, pad, gpu), _keep=(hi, lo))
    c["x64"], c["w64"] = C.join(c["hi"], c["lo"]), C.join(wh, wl)
    _CACHE[key] = c
    return c


def _ref(c, relu=False, leaky=None, res=False, addend=False):
    key = ("ref", relu, leaky, res, addend)
    if key not in c:
        c[key] = C.conv_fwd_ref(c["x64"], c["w64"], c["bias"], c["taps"], c["wp"], c["rows"], dil=c["dil"], relu=relu, leaky=leaky,
                                add=C.join(c["res"][0], c["res"][1]) if res else None, addend=c["addend"] if addend else None)
    return c[key]


def _launch(c, out_kw, relu=False, leaky=None, res=False, addend=False, border=False, repad=0, out_ld=0, tiling=0, tail=None):
    from magnet_amd import lib
    n = lib.conv_mfma(c["hi"], c["lo"], c["in_ld"], c["cin"], c["wh"], c["wl"], c["bias"], c["taps"], c["wp"], relu, c["rows"],
                      addend=c["addend"] if addend else None, dil=c["dil"] if c["dil"] > 1 else 0, out_ld=out_ld,
                      add=c["res"] if res else None, border=(c["hp"], c["pad"]) if border else None, repad=repad, leaky=leaky,
                      tiling=tiling, tail=tail, **out_kw)
    torch.cuda.synchronize()
    return n


def _run_plain(name, gpu, c, bm=128, out_wide=False, **kw):
    """One fp32 launch of case c checked against the reference image of its output buffer; returns the worst ratio."""
    border, repad = kw.get("border", False), kw.get("repad", 0)
    cout = c["cout"]
    out_ld, o0 = (cout + 16, 8) if out_wide else (cout, 0)
    ref, bound = _ref(c, **{k: v for k, v in kw.items() if k in ("relu", "leaky", "res", "addend")})
    if border:
        ref, bound, written = C.border_and_repad(ref, bound, c["N"], c["hp"], c["wp"], c["pad"], repad)
    else:
        written = c["inner"]                                          # plain form: border rows are unspecified, interior rows compared
    out_rows = ref.shape[0]
    buf, body = _guarded((out_rows + EXTRA, out_ld), gpu)
    tiles = _launch(c, dict(out_f32=body[:, o0:o0 + cout]), out_ld=out_ld, **kw)
    assert tiles == -(-c["rows"] // bm), f"{name}: {tiles} tiles: not the {bm}-row instance"
    _assert_untouched(name, buf, body, o0, o0 + cout, out_rows)
    got = body[:out_rows, o0:o0 + cout]
    worst = C.check(name, got[written], ref[written], bound[written])
    if border and repad:
        assert bool(_is_sentinel(got[~written]).all()), f"{name}: the target grid's border was written"
    print(f"[conv fwd {name}] rows={c['rows']} tiles={tiles} worst ratio {worst:.3f}")
    return worst


# ---- dispatch cases: plain epilogue, fp32 output ---------------------------------------------------------------------------------
GRID = dict(N=2, h=9, w=13)                       # 330 rows at border 1, 442 at border 2: three or four 128-row tiles, the last ragged
DISPATCH = [
    # id                                 cin  cout taps dil  extra
    ("nf8_win2-cout128-t9",              64,  128, 9,   1,   {}),
    ("nf8_win2-cout128-t9-dil2",         64,  128, 9,   2,   {}),
    ("nf8_win2-cout256-t9-gridy2",       64,  256, 9,   1,   {}),
    ("nf8_win1-cout128-t4",              64,  128, 4,   1,   {}),
    ("nf8_flat-cout128-t1",              64,  128, 1,   1,   {}),
    ("nf9_flat-cout144-t1",              64,  144, 1,   1,   {}),
    ("nf9_flat-cout144-t9",              64,  144, 9,   1,   {}),
    ("nf1_flat-cout16-t1",               64,  16,  1,   1,   {}),
    ("nf1_flat-cout16-t9",               64,  16,  9,   1,   {}),
    ("nf2_win2-cout32-t9",               64,  32,  9,   1,   {}),
    ("nf2_flat-cout32-t4",               64,  32,  4,   1,   {}),
    ("nf2_flat-cout32-t1",               64,  32,  1,   1,   {}),
    ("nf4_win2-cout64-t9",               64,  64,  9,   1,   {}),
    ("nf4_flat-cout64-t4",               64,  64,  4,   1,   {}),
    ("nf4_flat-cout64-t1",               64,  64,  1,   1,   {}),
    ("nf8_win2-cin32-one-chunk-per-tap", 32,  128, 9,   1,   {}),
    ("nf8_win2-cin320",                  320, 128, 9,   1,   {}),
    ("nf4_win2-cin32-dil2",              32,  64,  9,   2,   {}),
    ("nf2_win2-cin320",                  320, 32,  9,   1,   {}),
    ("nf8_win2-in_ld-gt-cin",            64,  128, 9,   1,   dict(in_wide=True)),
    ("nf4_flat-in_ld-gt-cin",            64,  64,  1,   1,   dict(in_wide=True)),
    ("nf8_win2-out_ld-gt-cout",          64,  128, 9,   1,   dict(out_wide=True)),
    ("nf1_flat-out_ld-gt-cout",          64,  16,  9,   1,   dict(out_wide=True)),
    ("nf8_win2-rows-lt-128",             64,  128, 9,   1,   dict(N=1, h=5, w=9)),        # 77 rows: one ragged tile
    ("nf8_win2-rows-256-exact",          64,  128, 9,   1,   dict(N=2, h=6, w=14)),       # 2 x 8 x 16 = 256 rows: no ragged tile
    ("nf9_flat-rows-256-exact",          64,  144, 9,   1,   dict(N=2, h=6, w=14)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,taps,dil,extra", [d[1:] for d in DISPATCH], ids=[d[0] for d in DISPATCH])
def test_plain_dispatch(hip_lib, gpu, request, cin, cout, taps, dil, extra):
    e = dict(extra)
    in_wide, out_wide = e.pop("in_wide", False), e.pop("out_wide", False)
    g = {**GRID, **e}
    c = _case(gpu, g["N"], g["h"], g["w"], max(dil, 1), cin, cout, taps, dil, in_wide=in_wide)
    if cout == 256:                               # grid.y = 2: the second block's weights and bias are its own
        assert not torch.equal(c["wh"][:, :128], c["wh"][:, 128:]) and not torch.equal(c["bias"][:128], c["bias"][128:])
    _run_plain(request.node.callspec.id, gpu, c, out_wide=out_wide)


@pytest.mark.gpu
def test_plain_8wave(hip_lib, gpu):
    """<8,2,256,0,512,PP,2>: cout_pad 128, 9 taps, fp32 output, no residual, no border and rows >= 65536 — the dispatch threshold,
    so 4 x 120 x 160 (79 056 rows, 309 tiles of 256 rows, the last one ragged) is about the smallest shape that reaches it; cin = 32
    keeps it one K chunk per tap.  The reference runs on the GPU in fp64."""
    c = _case(gpu, 4, 120, 160, 1, 32, 128, 9)
    assert c["rows"] == 79056 >= 65536 and c["rows"] % 256 != 0
    _run_plain("nf8_bm256_pp_win2-cout128-t9", gpu, c, bm=256)
    del _CACHE[next(k for k, v in _CACHE.items() if v is c)]          # 79 056-row fp64 tensors: not worth keeping


# ---- epilogue features -------------------------------------------------------------------------------------------------------------
FEATURES = [
    ("relu",            dict(relu=True), {}),
    ("leaky-neg-slope", dict(leaky=-0.3), {}),
    ("leaky-slope-gt1", dict(leaky=1.7), {}),
    ("residual-ld-gt-cout", dict(res=True, relu=True), {}),
    ("addend-ld-gt-cout",   dict(addend=True), {}),
    ("border",          dict(border=True, relu=True), {}),
    ("repad1",          dict(border=True, repad=1), {}),
    ("repad2",          dict(border=True, repad=2, res=True), {}),
    # 81 rows per image: a 128-row tile spans two and three images, the epilogue's `while (rem >= img_rows)` runs once and twice
    ("three-small-images-border", dict(border=True, leaky=-0.3), dict(N=3, h=5, w=5, pad=2)),
    ("three-small-images-repad2", dict(border=True, repad=2), dict(N=3, h=5, w=5, pad=2)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("form,cout", [("nf8_win2", 128), ("nf4_win2", 64)])
@pytest.mark.parametrize("kw,grid", [f[1:] for f in FEATURES], ids=[f[0] for f in FEATURES])
def test_epilogue_features(hip_lib, gpu, request, form, cout, kw, grid):
    g = {**GRID, "pad": 1, **grid}
    c = _case(gpu, g["N"], g["h"], g["w"], g["pad"], 64, cout, 9)
    _run_plain(request.node.callspec.id, gpu, c, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("form,cout", [("nf8_win2", 128), ("nf4_win2", 64)])
def test_output_modes(hip_lib, gpu, form, cout):
    """fp32, split planes and the single bf16 plane of one launch each over the same inputs (border zeroing on, ReLU, residual): the
    planes are split_bf16 of the fp32 output and the bf16 plane its round-to-nearest-even, bit for bit; border zeros are +0."""
    from magnet_amd.convnet import split_bf16
    c = _case(gpu, 2, 9, 13, 1, 64, cout, 9)
    kw = dict(relu=True, res=True, border=True)
    rows = c["rows"]
    ref, bound = _ref(c, relu=True, res=True)
    ref, bound, _ = C.border_and_repad(ref, bound, c["N"], c["hp"], c["wp"], c["pad"])
    bufs = {}
    for mode, dtype in (("f32", torch.float32), ("hi", torch.bfloat16), ("lo", torch.bfloat16), ("bf16", torch.bfloat16)):
        bufs[mode] = _guarded((rows + EXTRA, cout), gpu, dtype)
    _launch(c, dict(out_f32=bufs["f32"][1]), **kw)
    _launch(c, dict(out_hi=bufs["hi"][1], out_lo=bufs["lo"][1]), **kw)
    _launch(c, dict(out_bf16=bufs["bf16"][1]), **kw)
    for mode, (buf, body) in bufs.items():
        _assert_untouched(f"{form} {mode}", buf, body, 0, cout, rows)
    f32 = bufs["f32"][1][:rows]
    worst = C.check(f"{form} fp32", f32, ref, bound)
    eh, el = split_bf16(f32)
    C.check_planes_exact(f"{form} split planes", bufs["hi"][1][:rows], bufs["lo"][1][:rows], eh, el)
    assert torch.equal(bufs["bf16"][1][:rows].view(torch.int16), f32.to(torch.bfloat16).view(torch.int16)), f"{form}: bf16 plane is not RNE(fp32)"
    edge = ~c["inner"]
    assert bool((f32[edge].view(torch.int32) == 0).all()), "fp32 border outputs are not +0"
    for mode in ("hi", "lo", "bf16"):
        assert bool((bufs[mode][1][:rows][edge].view(torch.int16) == 0).all()), f"{mode} plane: border outputs are not +0"
    print(f"[conv fwd output modes {form}] worst ratio (fp32) {worst:.3f}; planes and bf16 plane bit-exact")


# ---- the fused tail --------------------------------------------------------------------------------------------------------------
def _tail_pack(gpu, tail_cout, seed=0):
    key = ("tail", tail_cout, seed)
    if key not in _CACHE:
        from magnet_amd.planes import pack_taps
        g = _g(50 + seed)
        ws = [(torch.randn(n, 128, 1, 1, generator=g) ** 3).abs() / 128 for n in (128, 128, tail_cout)]
        bs = [torch.randn(n, generator=g).abs() * 0.5 + 0.01 for n in (128, 128, tail_cout)]
        planes = [pack_taps(wv.to(gpu)) for wv in ws]
        t = dict(wh=torch.cat([p[0].reshape(-1) for p in planes]).contiguous(), wl=torch.cat([p[1].reshape(-1) for p in planes]).contiguous(),
                 bias=torch.cat(bs).to(gpu), cout=tail_cout)
        t["w64"] = C.join(t["wh"], t["wl"])
        _CACHE[key] = t
    return _CACHE[key]


TAILS = [
    # id                taps cin  addend tiling-bm256  rows per tile
    ("t9",              9,   64,  False, False,        128),
    ("bm256",           9,   64,  False, True,         256),          # 330 rows: the second 256-row tile is ragged
    ("addend-cin32",    9,   32,  True,  True,         128),          # the hoisted first layer stays on the 4-wave form under BM256
    ("addend-cin64",    9,   64,  True,  True,         128),
    ("t1",              1,   64,  False, False,        128),
    ("t4",              4,   64,  False, False,        128),
]


@pytest.mark.gpu
@pytest.mark.parametrize("tail_cout", [16, 128, 144])
@pytest.mark.parametrize("taps,cin,addend,bm256,bm", [t[1:] for t in TAILS], ids=[t[0] for t in TAILS])
def test_fused_tail(hip_lib, gpu, request, taps, cin, addend, bm256, bm, tail_cout):
    """3x3 / 2x2 / 1x1 first layer (bias, ReLU, addend) + the three fused 1x1 layers, every padded output channel compared."""
    from magnet_amd import lib
    name = request.node.callspec.id
    c = _case(gpu, 2, 9, 13, 1, cin, 128, taps)
    t = _tail_pack(gpu, tail_cout)
    a0, b0 = _ref(c, relu=True, addend=addend)
    ref, bound = C.tail_ref(a0, C.split_bound(a0, b0), t["w64"], t["bias"], tail_cout)
    buf, body = _guarded((c["rows"] + EXTRA, tail_cout), gpu)
    tiles = _launch(c, dict(out_f32=body), relu=True, addend=addend, tiling=lib.TILING_BM256 if bm256 else 0,
                    tail=(t["wh"], t["wl"], t["bias"], tail_cout))
    assert tiles == -(-c["rows"] // bm), f"{name}: {tiles} tiles: not the {bm}-row instance"
    _assert_untouched(name, buf, body, 0, tail_cout, c["rows"])
    inner = c["inner"]
    worst = C.check(name, body[:c["rows"]][inner], ref[inner], bound[inner])
    print(f"[conv fwd tail {name}] tiles={tiles} worst ratio {worst:.4f}")


# ---- addend + residual: rejected ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_addend_with_residual_is_rejected(hip_lib, gpu):
    """The epilogue holds one pre-bias term per channel; MagnetConvArgs documents the pair as excluded.  Every buffer is valid and
    full-size, and nothing is written."""
    from magnet_amd import lib
    c = _case(gpu, 2, 9, 13, 1, 64, 128, 9)
    buf, body = _guarded((c["rows"] + EXTRA, 128), gpu)
    for tiling in (None, 0):                      # magnet_conv_mfma and magnet_conv_mfma_ex
        with pytest.raises(lib.MagnetError, match="addend and add_hi/add_lo exclude each other") as ei:
            _launch(c, dict(out_f32=body), res=True, addend=True, tiling=tiling)
        assert ei.value.code == lib.E_DIM
    torch.cuda.synchronize()
    assert bool(_is_sentinel(buf).all())


# ---- magnet_pack_split, both kernels, bit for bit ------------------------------------------------------------------------------------
PACK = [
    # id                          N  C   h   w   ctot c_off extra
    ("wide-hw132",                2, 16, 11, 12, 16,  0,    {}),                          # two 128-pixel blocks, the second ragged
    ("wide-hw128",                2, 64, 8,  16, 64,  0,    {}),
    ("wide-C72-ragged-block",     2, 72, 11, 12, 72,  0,    {}),
    ("wide-c_off8-ctot96",        2, 64, 11, 12, 96,  8,    {}),
    ("wide-channel-slice-input",  2, 16, 11, 12, 32,  8,    dict(slice_of=24)),
    ("wide-nan-inf",              2, 16, 11, 12, 16,  0,    dict(nonfinite=True)),
    ("narrow-hw130",              2, 16, 10, 13, 16,  0,    {}),                          # 130 % 4 != 0: three 64-pixel blocks
    ("narrow-odd-hw65",           2, 8,  5,  13, 8,   0,    {}),
    ("narrow-C5",                 2, 5,  8,  16, 16,  0,    {}),
    ("narrow-C72-hw65",           1, 72, 5,  13, 96,  8,    {}),
    ("narrow-channel-slice-odd",  2, 13, 7,  9,  32,  8,    dict(slice_of=21)),
    ("narrow-unaligned-input",    2, 16, 11, 12, 16,  0,    dict(misalign=True)),
    ("narrow-nan-inf",            2, 5,  7,  9,  8,   0,    dict(nonfinite=True)),
]
PACK_FILL = -7.0                                  # a finite sentinel: NaN is an input here


@pytest.mark.gpu
@pytest.mark.parametrize("N,Cn,h,w,ctot,c_off,extra", [p[1:] for p in PACK], ids=[p[0] for p in PACK])
def test_pack_split(hip_lib, gpu, request, N, Cn, h, w, ctot, c_off, extra):
    """Both kernels of launch_pack_split against convnet.split_bf16 (Cn = the channel count C).  The wide kernel needs h*w % 4 == 0,
    C % 8 == 0, an image stride that is a multiple of 4 and a 16-byte aligned input; everything else takes the narrow one — so
    h*w = 130 is a narrow case (three 64-pixel blocks) and the wide kernel's ragged second 128-pixel block is reached at h*w = 132.
    Whole 8-channel vectors are stored: channels [C, round_up(C, 8)) of the destination are overwritten with +0 (the header's
    contract; ConvStackMFMA's in_map relies on it); border rows and every other channel keep their sentinel."""
    from magnet_amd import lib
    from magnet_amd.convnet import split_bf16
    name = request.node.callspec.id
    hw = h * w
    wide = hw % 4 == 0 and Cn % 8 == 0 and not extra.get("misalign") and (extra.get("slice_of", Cn) * hw) % 4 == 0
    assert wide == name.startswith("wide"), "the case does not reach the kernel its id names"
    Cfull = extra.get("slice_of", Cn)
    store = torch.randn(N * Cfull * hw + 4, generator=_g(70 + Cn + hw))
    if extra.get("nonfinite"):
        store[3::17] = float("nan"); store[5::23] = float("inf"); store[7::29] = float("-inf")
    store = store.to(gpu)
    o = 1 if extra.get("misalign") else 0
    x = store[o:o + N * Cfull * hw].view(N, Cfull, h, w)[:, :Cn]
    assert (x.data_ptr() % 16 == 0) == (not extra.get("misalign"))
    c8 = -(-Cn // 8) * 8
    bufs = [_guarded((N, h + 2, w + 2, ctot), gpu, torch.bfloat16, PACK_FILL) for _ in range(2)]
    lib.pack_split(x, bufs[0][1], bufs[1][1], ctot, c_off)
    torch.cuda.synchronize()
    xp = torch.zeros((N, h, w, c8), dtype=torch.float32, device=gpu)
    xp[..., :Cn] = x.permute(0, 2, 3, 1)
    eh, el = split_bf16(xp)
    exp = [torch.full((N, h + 2, w + 2, ctot), PACK_FILL, dtype=torch.bfloat16, device=gpu) for _ in range(2)]
    for e, pl in zip(exp, (eh, el)):
        e[:, 1:-1, 1:-1, c_off:c_off + c8] = pl
    C.check_planes_exact(name, bufs[0][1], bufs[1][1], exp[0], exp[1])          # interior, border rows and the other channels
    for buf, _ in bufs:
        fill = torch.full((GUARD,), PACK_FILL, dtype=torch.bfloat16, device=gpu)
        assert torch.equal(buf[:GUARD], fill) and torch.equal(buf[-GUARD:], fill), f"{name}: write outside the buffer"
    if c8 > Cn:                                    # the round-up lanes: +0 in both planes, bit for bit
        for _, body in bufs:
            assert bool((body[:, 1:-1, 1:-1, c_off + Cn:c_off + c8].contiguous().view(torch.int16) == 0).all())
    if extra.get("nonfinite"):
        assert bool(torch.isnan(bufs[0][1].float()).any() and torch.isinf(bufs[0][1].float()).any())
