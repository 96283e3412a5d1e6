"""The single-plane fp16 operand format (magnet_conv_mfma_f16, magnet_pack_f16, magnet_planes_to_f16), one direct launch per case.

Built like tests/test_gpu_conv_fwd.py, whose helpers and fp64 reference (tests/conv_fwd_ref.py) are imported, not copied: NaN guard
bands and sentinel checks around every output, heavy-tailed inputs, every padded output channel compared.

Pointwise bound of the 3x3 layer.  The reference is the fp64 convolution of exactly the fp16 planes the kernel received, so every
product x w is exact in the fp32 accumulator (11 x 11 significant bits) and nothing is dropped: what is left is the accumulation,
K = taps * cin roundings, and the epilogue's additions — the accumulator starts at the addend, the bias is added after the loop — inside
L = K + 4:  |pre - ref| <= gamma(K + 4) (|x| conv |w| + |addend| + |bias|).  Derived, not measured.  ReLU is 1-Lipschitz.  Behind the
fused tail the bound is carried through the three bf16x3 1x1 layers by conv_fwd_ref.split_bound / tail_ref, as in test_fused_tail.

Instances of launch_conv_mfma_f16 (csrc/conv_mfma.hip), all <NF 8, WN 2, WIN 2>:
  fused tail T = 1 / 9, rows >= 65536 or TILING_BM256, no addend    <256 rows, 512 threads, PP>    test_f16_fused_tail[bm256-*]
  fused tail T = 1 / 9 otherwise (so: every launch with an addend)   <128 rows, 256 threads>        test_f16_fused_tail[t9-*], [addend-*], [slice-*]
  plain fp32 output, rows >= 65536 or TILING_BM256                   <256 rows, 512 threads, PP>    test_f16_plain_8wave, test_f16_plain[bm256]
  plain fp32 output otherwise                                        <128 rows, 256 threads>        test_f16_plain[t9], [addend], [slice]
The tile count the library reports is asserted in each.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_fwd_ref as C
from tests.test_conv_precision_host import EDGE_VALUES, assert_f16_bits_equal, f16_sat_bits, planes_sum_f32
from tests.test_gpu_conv_fwd import EXTRA, GUARD, _CACHE, _assert_untouched, _case, _g, _guarded, _heavy, _is_sentinel, _tail_pack


def _bits(t):
    """uint16 bit patterns of a 2-byte tensor, on the host."""
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _case16(gpu, cin, sliced=False, big=False):
    """The fp16 planes of test_gpu_conv_fwd._case(gpu, 2, 9, 13, 1, cin, 128, 9) (330 rows) — activations f16(hi + lo), weights
    f16(hi + lo) — and what the reference needs, built once.  sliced: the cin channels sit at channel 64 of a 320-wide buffer whose
    other channels hold data, not zeros.  big: the 79 056-row shape of test_plain_8wave."""
    key = ("f16", cin, sliced, big)
    if key in _CACHE:
        return _CACHE[key]
    from magnet_amd.planes import to_f16_sat
    c = _case(gpu, 4, 120, 160, 1, cin, 128, 9) if big else _case(gpu, 2, 9, 13, 1, cin, 128, 9)
    x16 = to_f16_sat((c["hi"].float() + c["lo"].float()))
    if sliced:
        buf = to_f16_sat(torch.randn((c["rows"], 320), generator=_g(90)).to(gpu))
        buf[:, 64:64 + cin] = x16
        x16, in_ld, keep = buf[:, 64:64 + cin], 320, buf
    else:
        x16 = x16.contiguous()
        in_ld, keep = cin, x16
    w16 = to_f16_sat(c["wh"].float() + c["wl"].float()).contiguous()
    K = 9 * cin
    ref, b0 = C.conv_ref(x16.double(), w16.double(), 9, c["wp"], c["rows"])
    mag = b0 / (1.01 * C.LOLO + 1.02 * C.gamma_l(3 * K + 2))           # conv_ref's |x| conv |w|
    d = dict(c=c, x16=x16, in_ld=in_ld, w16=w16, cin=cin, rows=c["rows"], wp=c["wp"], bias=c["bias"], addend=c["addend"], inner=c["inner"],
             conv=ref, mag=mag, K=K, _keep=keep)
    _CACHE[key] = d
    return d


def _ref16(d, relu, addend):
    """(ref, bound) of the 3x3 layer's fp32 result: see the module docstring."""
    bias = d["bias"].double()[:128]
    terms = bias.abs().expand_as(d["conv"]).clone()
    ref = d["conv"]
    if addend:
        a = d["addend"][:d["rows"], :128].double()
        ref, terms = ref + a, terms + a.abs()
    ref = ref + bias
    bound = C.gamma_l(d["K"] + 4) * (d["mag"] + terms)
    return (ref.clamp_min(0.0) if relu else ref), bound


def _launch16(d, relu=False, addend=False, tiling=0, **kw):
    from magnet_amd import lib
    n = lib.conv_mfma(d["x16"], None, d["in_ld"], d["cin"], d["w16"], None, d["bias"], 9, d["wp"], relu, d["rows"],
                      addend=d["addend"] if addend else None, tiling=tiling, f16=True, **kw)
    torch.cuda.synchronize()
    return n


CASES = [
    # id        cin  sliced addend bm256  rows per tile
    ("t9",      64,  False, False, False, 128),
    ("bm256",   64,  False, False, True,  256),          # 330 rows: the second 256-row tile is ragged
    ("addend",  64,  False, True,  True,  128),          # a launch with an addend stays on the 4-wave form under BM256
    ("slice",   256, True,  False, False, 128),          # channels [64, 320) of a 320-wide buffer: in_ld 320
    ("slice-addend", 256, True, True, False, 128),
]


@pytest.mark.gpu
@pytest.mark.parametrize("tail_cout", [16, 144])
@pytest.mark.parametrize("cin,sliced,addend,bm256,bm", [t[1:] for t in CASES], ids=[t[0] for t in CASES])
def test_f16_fused_tail(hip_lib, gpu, request, cin, sliced, addend, bm256, bm, tail_cout):
    """fp16 3x3 layer (bias, ReLU, addend) + the three fused bf16x3 1x1 layers."""
    from magnet_amd import lib
    name = request.node.callspec.id
    d = _case16(gpu, cin, sliced)
    t = _tail_pack(gpu, tail_cout)
    a0, b0 = _ref16(d, True, addend)
    ref, bound = C.tail_ref(a0, C.split_bound(a0, b0), t["w64"], t["bias"], tail_cout)
    buf, body = _guarded((d["rows"] + EXTRA, tail_cout), gpu)
    tiles = _launch16(d, relu=True, addend=addend, tiling=lib.TILING_BM256 if bm256 else 0, out_f32=body,
                      tail=(t["wh"], t["wl"], t["bias"], tail_cout))
    assert tiles == -(-d["rows"] // bm), f"{name}: {tiles} tiles: not the {bm}-row instance"
    _assert_untouched(name, buf, body, 0, tail_cout, d["rows"])
    inner = d["inner"]
    worst = C.check(name, body[:d["rows"]][inner], ref[inner], bound[inner])
    print(f"[conv f16 tail {name}] tiles={tiles} worst ratio {worst:.4f}")


PLAIN = [("t9", 64, False, False, False, 128), ("addend", 64, False, True, False, 128), ("slice", 256, True, False, False, 128),
         ("bm256", 64, False, False, True, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,sliced,addend,bm256,bm", [t[1:] for t in PLAIN], ids=[t[0] for t in PLAIN])
def test_f16_plain(hip_lib, gpu, request, cin, sliced, addend, bm256, bm):
    """The plain fp32-output form (run_invariant's launch: no bias worth the name, no ReLU — here with the case's random bias)."""
    from magnet_amd import lib
    name = request.node.callspec.id
    d = _case16(gpu, cin, sliced)
    ref, bound = _ref16(d, False, addend)
    buf, body = _guarded((d["rows"] + EXTRA, 128), gpu)
    tiles = _launch16(d, addend=addend, tiling=lib.TILING_BM256 if bm256 else 0, out_f32=body)
    assert tiles == -(-d["rows"] // bm), f"{name}: {tiles} tiles: not the {bm}-row instance"
    _assert_untouched(name, buf, body, 0, 128, d["rows"])
    inner = d["inner"]
    worst = C.check(name, body[:d["rows"]][inner], ref[inner], bound[inner])
    print(f"[conv f16 plain {name}] tiles={tiles} worst ratio {worst:.4f}")


@pytest.mark.gpu
def test_f16_plain_8wave(hip_lib, gpu):
    """The 8-wave form at its own threshold: the 79 056 rows of test_plain_8wave (309 tiles of 256 rows, the last ragged), cin 32."""
    d = _case16(gpu, 32, big=True)
    assert d["rows"] == 79056
    ref, bound = _ref16(d, False, False)
    buf, body = _guarded((d["rows"] + EXTRA, 128), gpu)
    tiles = _launch16(d, out_f32=body)
    assert tiles == -(-d["rows"] // 256)
    _assert_untouched("plain-8wave", buf, body, 0, 128, d["rows"])
    inner = d["inner"]
    worst = C.check("plain-8wave", body[:d["rows"]][inner], ref[inner], bound[inner])
    print(f"[conv f16 plain 8-wave] tiles={tiles} worst ratio {worst:.4f}")
    for k in [k for k, v in _CACHE.items() if v is d or v is d["c"]]:
        del _CACHE[k]                                                   # 79 056-row fp64 tensors: not worth keeping


# ---- the fused Gaussian update and the fused upsampling: bit for bit the plain tail + the stand-alone kernel ---------------------
def _gmm(gpu, B, h, w, seed):
    g = _g(seed)
    return torch.cat([torch.rand(B, 1, h, w, generator=g) * 5 + 0.5, torch.rand(B, 1, h, w, generator=g) * 0.5 + 0.05], dim=1).to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("bm256", [False, True], ids=["bm128", "bm256"])
def test_f16_fused_gaussian_update_equals_the_two_launch_form(hip_lib, gpu, bm256):
    from magnet_amd import lib
    d = _case16(gpu, 64)
    t = _tail_pack(gpu, 16)
    tail = (t["wh"], t["wl"], t["bias"], 16)
    tiling = lib.TILING_BM256 if bm256 else 0
    gmm = _gmm(gpu, 2, 9, 13, 31)
    o = torch.empty((d["rows"], 16), dtype=torch.float32, device=gpu)
    _launch16(d, relu=True, tiling=tiling, out_f32=o, tail=tail)
    ref = lib.gaussian_update_cl(o, 16, gmm, 9, 13)
    buf, out = _guarded(tuple(gmm.shape), gpu)
    _launch16(d, relu=True, tiling=tiling, tail=tail, gauss=(gmm, out))
    assert bool(_is_sentinel(buf[:GUARD]).all() and _is_sentinel(buf[-GUARD:]).all())
    assert torch.equal(out, ref), f"max|d| = {(out - ref).abs().max().item():.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("bm256", [False, True], ids=["bm128", "bm256"])
def test_f16_fused_upsampling_equals_the_two_launch_form(hip_lib, gpu, bm256):
    from magnet_amd import lib
    d = _case16(gpu, 256, sliced=True)
    t = _tail_pack(gpu, 144)
    tail = (t["wh"], t["wl"], t["bias"], 144)
    tiling = lib.TILING_BM256 if bm256 else 0
    depths = [_gmm(gpu, 2, 9, 13, 33), _gmm(gpu, 2, 9, 13, 34)]
    mask = torch.empty((d["rows"], 144), dtype=torch.float32, device=gpu)
    _launch16(d, relu=True, tiling=tiling, out_f32=mask, tail=tail)
    ref = torch.stack(lib.upsample_depth_cl_n(depths, mask, 144))
    buf, outs = _guarded((2, 2, 2, 36, 52), gpu)
    _launch16(d, relu=True, tiling=tiling, tail=tail, upsample=(torch.stack(depths), outs))
    assert bool(_is_sentinel(buf[:GUARD]).all() and _is_sentinel(buf[-GUARD:]).all())
    assert torch.equal(outs, ref), f"max|d| = {(outs - ref).abs().max().item():.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w,bm256,tiles,by_image", [(3, 9, 13, False, 4, False), (3, 9, 13, True, 2, False), (5, 32, 14, True, 10, True)])
def test_f16_per_image_tiling_equals_flat(hip_lib, gpu, B, h, w, bm256, tiles, by_image):
    """Per-image tiling against MAGNET_TILING_FLAT, fused Gaussian update, bit for bit.  At B = 3, h = 9, w = 13 the rule keeps the
    flat form on both tile sizes (4 and 2 tiles); 5 x 32 x 14 on 256-row tiles is tiled per image (10 tiles, flat 11)."""
    from magnet_amd import lib
    from magnet_amd.planes import to_f16_sat
    rows, wp = B * (h + 2) * (w + 2), w + 2
    x = torch.zeros((B, h + 2, wp, 64))
    x[:, 1:-1, 1:-1] = _heavy((B, h, w, 64), 95)
    d0 = _case16(gpu, 64)
    d = dict(d0, x16=to_f16_sat(x.reshape(rows, 64).to(gpu)), rows=rows, wp=wp, in_ld=64)
    t = _tail_pack(gpu, 16)
    gmm = _gmm(gpu, B, h, w, 35)
    base = lib.TILING_BM256 if bm256 else 0
    res = {}
    for name, tiling in (("auto", base), ("flat", base | lib.TILING_FLAT)):
        buf, out = _guarded(tuple(gmm.shape), gpu)
        n = _launch16(d, relu=True, tiling=tiling, tail=(t["wh"], t["wl"], t["bias"], 16), gauss=(gmm, out))
        assert bool(_is_sentinel(buf[:GUARD]).all() and _is_sentinel(buf[-GUARD:]).all()), f"{name}: write outside the output"
        assert not torch.isnan(out).any(), f"{name}: interior positions left unwritten"
        res[name] = (n, out.clone())
    flat_tiles = -(-rows // (256 if bm256 else 128))
    assert res["flat"][0] == flat_tiles and res["auto"][0] == tiles and (tiles < flat_tiles) == by_image
    assert torch.equal(res["auto"][1], res["flat"][1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_f16_refusals(hip_lib, gpu):
    """A non-NULL in_lo, taps 1, MAGNET_TILING_BM64 and a residual each return MAGNET_E_DIM, and nothing is written.  The valid
    launch they are one field away from is made first."""
    from magnet_amd import lib
    d = _case16(gpu, 64)
    buf, body = _guarded((d["rows"] + EXTRA, 128), gpu)
    res = torch.zeros((d["rows"], 128), dtype=torch.bfloat16, device=gpu)

    def args(**over):
        a = lib.MagnetConvArgs()
        a.in_hi, a.w_hi, a.bias, a.out_f32 = d["x16"].data_ptr(), d["w16"].data_ptr(), d["bias"].data_ptr(), body.data_ptr()
        a.rows, a.cin, a.cout_pad, a.taps, a.wp, a.out_mode, a.in_ld = d["rows"], 64, 128, 9, d["wp"], 1, 64
        tiling = over.pop("tiling", 0)
        for k, v in over.items():
            setattr(a, k, v)
        return lib.MagnetConvExArgs(base=a, tiling=tiling)

    f = lib.load().magnet_conv_mfma_f16
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    with torch.cuda.device(gpu):
        assert f(ctypes.byref(args()), stream) == 0
        torch.cuda.synchronize()
        assert not bool(_is_sentinel(body[:d["rows"]]).any())
        body.fill_(float("nan"))
        for name, over in (("in_lo", dict(in_lo=d["x16"].data_ptr())), ("w_lo", dict(w_lo=d["w16"].data_ptr())), ("taps 1", dict(taps=1)),
                           ("BM64", dict(tiling=lib.TILING_BM64)), ("residual", dict(add_hi=res.data_ptr(), add_lo=res.data_ptr())),
                           ("out_mode 0", dict(out_mode=0, out_hi=res.data_ptr(), out_lo=res.data_ptr())), ("cout_pad 64", dict(cout_pad=64))):
            assert f(ctypes.byref(args(**over)), stream) == lib.E_DIM, name
        torch.cuda.synchronize()
    assert bool(_is_sentinel(buf).all())


# ---- magnet_pack_f16 (csrc/pack.hip: pack_nchw_kernel<PackF16, 128> in the "wide" cases, <PackF16, 64> in the "narrow" ones) and
# ---- magnet_planes_to_f16, bit for bit against the host restatement
PACK_FILL = -7.0                                  # a finite sentinel: NaN is an input here
PACK = [
    # id                       N  C   h   w   ctot c_off
    ("wide-hw132",             2, 16, 11, 12, 16,  0),       # two 128-pixel blocks, the second ragged
    ("wide-C72-c_off64-ctot320", 2, 72, 11, 12, 320, 64),    # a ragged second channel block, a non-zero c_off in a wider buffer
    ("narrow-hw130",           2, 16, 10, 13, 16,  0),       # 130 % 4 != 0
    ("narrow-C5-c_off8",       2, 5,  7,  9,  32,  8),       # odd h*w, C % 8 != 0: the round-up lanes are written as +0
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,Cn,h,w,ctot,c_off", [p[1:] for p in PACK], ids=[p[0] for p in PACK])
def test_pack_f16(hip_lib, gpu, request, N, Cn, h, w, ctot, c_off):
    from magnet_amd import lib
    name = request.node.callspec.id
    assert ((h * w) % 4 == 0 and Cn % 8 == 0) == name.startswith("wide"), "the case does not reach the kernel its id names"
    x = (torch.randn(N, Cn, h, w, generator=_g(70 + Cn)) * torch.exp2(torch.randint(-28, 18, (N, Cn, h, w), generator=_g(71)).float()))
    flat = x.view(-1)
    flat[3::17] = float("nan")
    flat[:EDGE_VALUES.size] = torch.from_numpy(EDGE_VALUES)
    flat[100:100 + EDGE_VALUES.size] = -torch.from_numpy(EDGE_VALUES)
    buf, body = _guarded((N, h + 2, w + 2, ctot), gpu, torch.float16, PACK_FILL)
    lib.pack_f16(x.to(gpu), body, ctot, c_off)
    torch.cuda.synchronize()
    c8 = -(-Cn // 8) * 8
    fill = _bits(torch.tensor([PACK_FILL], dtype=torch.float16))[0]
    exp = np.full((N, h + 2, w + 2, ctot), fill, dtype=np.uint16)
    xp = np.zeros((N, h, w, c8), dtype=np.float32)
    xp[..., :Cn] = x.permute(0, 2, 3, 1).numpy()
    exp[:, 1:-1, 1:-1, c_off:c_off + c8] = f16_sat_bits(xp)
    assert_f16_bits_equal(name, _bits(body), exp)                      # interior, border rows and every other channel
    assert bool((_bits(buf[:GUARD]) == fill).all() and (_bits(buf[-GUARD:]) == fill).all()), f"{name}: write outside the buffer"


@pytest.mark.gpu
@pytest.mark.parametrize("c0,c1", [(0, 64), (64, 320)])
def test_planes_to_f16(hip_lib, gpu, c0, c1):
    """330 rows of a 320-wide split-bf16 buffer -> the same channels of a 320-wide fp16 plane; planes that are the split of fp32
    values (edge values included: hi + lo is then that value) and, in the last rows, arbitrary bf16 pairs."""
    from magnet_amd import lib
    from magnet_amd.convnet import split_bf16
    rows, ld = 330, 320
    x = torch.randn(rows, ld, generator=_g(80)) * torch.exp2(torch.randint(-28, 18, (rows, ld), generator=_g(81)).float())
    x.view(-1)[5::19] = float("nan")
    x[7, :EDGE_VALUES.size] = torch.from_numpy(EDGE_VALUES)
    x[8, 64:64 + EDGE_VALUES.size] = -torch.from_numpy(EDGE_VALUES)
    hi, lo = split_bf16(x.to(gpu))
    lo[-4:] = torch.randn(4, ld, generator=_g(82)).to(gpu).to(torch.bfloat16)
    buf, body = _guarded((rows, ld), gpu, torch.float16, PACK_FILL)
    lib.planes_to_f16(hi, lo, body, c0, c1)
    torch.cuda.synchronize()
    fill = _bits(torch.tensor([PACK_FILL], dtype=torch.float16))[0]
    exp = np.full((rows, ld), fill, dtype=np.uint16)
    exp[:, c0:c1] = f16_sat_bits(planes_sum_f32(_bits(hi), _bits(lo)))[:, c0:c1]
    assert_f16_bits_equal(f"planes_to_f16 [{c0}, {c1})", _bits(body), exp)
    assert bool((_bits(buf[:GUARD]) == fill).all() and (_bits(buf[-GUARD:]) == fill).all())
