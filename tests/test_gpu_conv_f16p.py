"""magnet_conv_mfma_f16p, the single-plane fp16 format "plane to plane" (the F-Net's launches), one direct launch per case.

Built like tests/test_gpu_conv_f16.py: the helpers of tests/test_gpu_conv_fwd.py and the fp64 reference of tests/conv_fwd_ref.py are
imported, not copied; NaN guard bands and sentinel checks around every output, heavy-tailed inputs, every padded channel compared.

Shape: N = 2, h = 9, w = 13 on a border of 2 = 2 x 13 x 17 = 442 rows: four 128-row tiles, the last ragged, an image boundary inside a
tile.  The tile count the library reports (rows / 128 rounded up: the 128-row 4-wave instances) is asserted in every case.

Bound.  The reference is the fp64 convolution of exactly the fp16 planes passed in, so every product x w is exact in the fp32
accumulator (11 x 11 significant bits).  What is left: K = taps * cin accumulator roundings and the epilogue's additions (residual,
bias), inside L = K + 4:
    fp32 output      |out - ref| <= gamma(K + 4) (|x| conv |w| + |res| + |bias|)                         (as test_gpu_conv_f16, + the residual)
    fp16 plane       + one fp16 rounding of the result: 2^-11 |ref| where |ref| >= 2^-14, else 2^-25
    single bf16      + one bf16 rounding (8 significant bits: spacing 2^(e-7) in [2^e, 2^(e+1)), half of it <= 2^-8 |v|) of the fp32
                     result v, |v| <= |ref| + the fp32 bound: 2^-8 (|ref| + the fp32 bound)
The fp16 residual plane is converted to fp32 exactly.  ReLU is 1-Lipschitz and maps 0 to 0.  Derived, not measured.

Instances of launch_conv_mfma_f16p (csrc/conv_mfma.hip), all 128 rows x 256 threads, F16P:
    taps 9, cout_pad 128 / 64 / 32   <NF 8, WN 2 | 4, 1 | 2, 1; WIN 2>   t9-*  (cout 32: one weight DMA piece per wave)
    taps 4 / 1, the same widths      <... WIN 0>                           t4-*, t1-*
"""
import pytest
import torch

from tests import conv_fwd_ref as C
from tests.test_gpu_conv_fwd import EXTRA, GUARD, _CACHE, _case, _g, _guarded

SENT = {torch.float32: (torch.int32, 0x7FC00000), torch.bfloat16: (torch.int16, 0x7FC0), torch.float16: (torch.int16, 0x7E00)}
N, H, W, PAD = 2, 9, 13, 2


def _sent(t):
    """Elementwise: still the NaN the buffer was filled with, bit for bit (fp32, bf16 and fp16 buffers)."""
    it, bits = SENT[t.dtype]
    return t.contiguous().view(it) == bits


def _case16(gpu, cin, cout, taps, dil=1, in_slice=False):
    """fp16 planes of test_gpu_conv_fwd._case (activations f16(hi + lo), weights f16(hi + lo), residual f16(rh + rl)) and the fp64
    pieces of the reference, built once and never modified.  in_slice: the cin channels are channels [64, 64 + cin) of a 320-wide
    plane whose other channels hold data, not zeros."""
    key = ("f16p", cin, cout, taps, dil, in_slice)
    if key in _CACHE:
        return _CACHE[key]
    from magnet_amd.planes import to_f16_sat
    c = _case(gpu, N, H, W, PAD, cin, cout, taps, dil)
    x16 = to_f16_sat(c["hi"].float() + c["lo"].float())
    if in_slice:
        buf = to_f16_sat(torch.randn((c["rows"], 320), generator=_g(91)).to(gpu))
        buf[:, 64:64 + cin] = x16
        x16, in_ld, keep = buf[:, 64:64 + cin], 320, buf
    else:
        x16 = x16.contiguous()
        in_ld, keep = cin, x16
    w16 = to_f16_sat(c["wh"].float() + c["wl"].float()).contiguous()
    r16 = to_f16_sat(c["res"][0].float() + c["res"][1].float()).contiguous()          # (rows, cout + 8): add_ld = cout + 8
    K = taps * cin
    conv, b0 = C.conv_ref(x16.double(), w16.double(), taps, c["wp"], c["rows"], dil)
    mag = b0 / (1.01 * C.LOLO + 1.02 * C.gamma_l(3 * K + 2))                           # conv_ref's |x| conv |w|
    d = dict(c=c, x16=x16, in_ld=in_ld, w16=w16, r16=r16, cin=cin, cout=cout, taps=taps, dil=dil, rows=c["rows"], wp=c["wp"],
             hp=c["hp"], bias=c["bias"], inner=c["inner"], conv=conv, mag=mag, K=K, _keep=keep)
    _CACHE[key] = d
    return d


def _ref(d, relu, res):
    """(ref, bound) of the fp32 result: see the module docstring."""
    bias = d["bias"].double()[:d["cout"]]
    ref, terms = d["conv"], bias.abs().expand_as(d["conv"]).clone()
    if res:
        r = d["r16"][:d["rows"], :d["cout"]].double()
        ref, terms = ref + r, terms + r.abs()
    ref = ref + bias
    bound = C.gamma_l(d["K"] + 4) * (d["mag"] + terms)
    return (ref.clamp_min(0.0) if relu else ref), bound


def _f16_bound(ref, bound):
    """One fp16 rounding of the result on top of the fp32 bound."""
    a = ref.abs()
    return bound + torch.where(a >= 2.0 ** -14, a * 2.0 ** -11, torch.full_like(a, 2.0 ** -25))


def _launch(d, relu, res, **kw):
    from magnet_amd import lib
    n = lib.conv_mfma(d["x16"], None, d["in_ld"], d["cin"], d["w16"], None, d["bias"], d["taps"], d["wp"], relu, d["rows"],
                      dil=d["dil"] if d["dil"] > 1 else 0, add=(d["r16"], None, d["cout"] + 8) if res else None, f16="plane", **kw)
    torch.cuda.synchronize()
    return n


def _untouched(name, buf, body, c0, c1, rows_written):
    assert bool(_sent(buf[:GUARD]).all() and _sent(buf[-GUARD:]).all()), f"{name}: write outside the output buffer"
    assert bool(_sent(body[rows_written:]).all()), f"{name}: a row at or past `rows` was written"
    assert bool(_sent(body[:, :c0]).all() and _sent(body[:, c1:]).all()), f"{name}: a channel outside the slice was written"


MODES = [("plain", False, False), ("relu", True, False), ("res", False, True), ("res-relu", True, True)]
CASES = [
    # id                cin  cout taps dil  in_slice out_slice
    *[(f"t9-{ci}x{co}", ci,  co,  9,   1,   False,   False) for ci in (32, 64, 128) for co in (32, 64, 128)],
    ("t9-dil2-128x128", 128, 128, 9,   2,   False,   False),
    ("t9-dil2-64x64",   64,  64,  9,   2,   False,   False),
    ("t9-dil2-32x32",   32,  32,  9,   2,   False,   False),
    ("t9-in-slice",     128, 128, 9,   1,   True,    False),        # channels [64, 192) of a 320-wide plane
    ("t9-cin320",       320, 128, 9,   1,   False,   False),        # lastconv.0
    ("t9-out-slice128", 128, 128, 9,   1,   False,   True),         # writes channels [64, 192) of a 320-wide plane
    ("t9-out-slice64",  64,  64,  9,   1,   False,   True),
    ("t1-64x128",       64,  128, 1,   1,   False,   False),        # projection shortcut
    ("t1-128x64",       128, 64,  1,   1,   False,   False),
    ("t4-128x64",       128, 64,  4,   1,   False,   False),        # layer2.0.conv1 over the space-to-depth tensor
    ("t4-128x32",       128, 32,  4,   1,   False,   False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,relu,res", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("cin,cout,taps,dil,in_slice,out_slice", [t[1:] for t in CASES], ids=[t[0] for t in CASES])
def test_f16p_plane_output(hip_lib, gpu, request, cin, cout, taps, dil, in_slice, out_slice, mode, relu, res):
    """fp16 plane in, fp16 plane out, with the zero border (border=(hp, 2)): the F-Net's layer-to-layer form."""
    name = request.node.callspec.id
    d = _case16(gpu, cin, cout, taps, dil, in_slice)
    ref, bound = _ref(d, relu, res)
    ref, bound, written = C.border_and_repad(ref, _f16_bound(ref, bound), N, d["hp"], d["wp"], PAD, 0)
    out_ld, o0 = (320, 64) if out_slice else (cout, 0)
    buf, body = _guarded((d["rows"] + EXTRA, out_ld), gpu, torch.float16)
    tiles = _launch(d, relu, res, out_hi=body[:, o0:o0 + cout], out_ld=out_ld, border=(d["hp"], PAD))
    assert tiles == -(-d["rows"] // 128), f"{name}: {tiles} tiles: not a 128-row instance"
    _untouched(name, buf, body, o0, o0 + cout, d["rows"])
    got = body[:d["rows"], o0:o0 + cout]
    worst = C.check(name, got, ref, bound)
    border = got[~d["inner"]]
    assert bool((border.contiguous().view(torch.int16) == 0).all()), f"{name}: a border position is not +0"
    print(f"[conv f16p {name}] tiles={tiles} worst ratio {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,relu,res", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("cin,cout,taps", [(128, 32, 1), (64, 128, 1), (128, 64, 4), (64, 32, 9)], ids=["t1-128x32", "t1-64x128", "t4-128x64", "t9-64x32"])
def test_f16p_fp32_output(hip_lib, gpu, request, cin, cout, taps, mode, relu, res):
    """fp32 output without a border (the SPP branches' 1x1 layer: out_mode 1), interior rows compared."""
    name = request.node.callspec.id
    d = _case16(gpu, cin, cout, taps)
    ref, bound = _ref(d, relu, res)
    buf, body = _guarded((d["rows"] + EXTRA, cout), gpu)
    tiles = _launch(d, relu, res, out_f32=body)
    assert tiles == -(-d["rows"] // 128)
    _untouched(name, buf, body, 0, cout, d["rows"])
    inner = d["inner"]
    worst = C.check(name, body[:d["rows"]][inner], ref[inner], bound[inner])
    print(f"[conv f16p fp32 {name}] tiles={tiles} worst ratio {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("repad", [1, 2])
@pytest.mark.parametrize("out", ["fp32", "bf16"])
@pytest.mark.parametrize("cout", [64, 32])
def test_f16p_repad_outputs(hip_lib, gpu, request, cout, out, repad):
    """lastconv.2 into the matcher's layouts: taps 1 over 128 channels, interior rows re-addressed to a grid with border repad - 1,
    fp32 or one bf16 plane; the target grid's border and everything else keep their sentinel."""
    name = request.node.callspec.id
    d = _case16(gpu, 128, cout, 1)
    ref, bound = _ref(d, False, False)
    dt = torch.float32 if out == "fp32" else torch.bfloat16
    if out == "bf16":
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    ref, bound, written = C.border_and_repad(ref, bound, N, d["hp"], d["wp"], PAD, repad)
    buf, body = _guarded((ref.shape[0] + EXTRA, cout), gpu, dt)
    kw = dict(out_f32=body) if out == "fp32" else dict(out_bf16=body)
    tiles = _launch(d, False, False, border=(d["hp"], PAD), repad=repad, out_ld=cout, **kw)
    assert tiles == -(-d["rows"] // 128)
    _untouched(name, buf, body, 0, cout, ref.shape[0])
    got = body[:ref.shape[0]]
    worst = C.check(name, got[written], ref[written], bound[written])
    assert bool(_sent(got[~written]).all()), f"{name}: the target grid's border was written"
    print(f"[conv f16p repad {name}] worst ratio {worst:.4f}")


@pytest.mark.gpu
def test_f16p_store_saturates_and_nan_passes_through(hip_lib, gpu):
    """Operands at the format's edge: a row of 32 x 65504 against weights +1 / -1 / +2^-5 sums to +-2 096 128 and 65504 in fp32; the fp16
    store clamps the first two to +-65504 (never Inf) and keeps the third; with ReLU the negative one is +0.  A NaN operand makes its
    whole output row NaN (0 x NaN = NaN in the matrix instruction) and the store writes NaN through."""
    from magnet_amd import lib
    rows, cin, cout = 130, 32, 32                                                   # two tiles, the second ragged
    x = torch.zeros((rows, cin), dtype=torch.float16)
    x[0] = 65504.0
    x[1, 3] = float("nan")
    x[129] = -65504.0
    w = torch.zeros((1, cout, cin), dtype=torch.float16)
    w[0, 0], w[0, 1], w[0, 2] = 1.0, -1.0, 2.0 ** -5
    bias = torch.zeros(cout)
    for relu in (False, True):
        buf, body = _guarded((rows + EXTRA, cout), gpu, torch.float16)
        lib.conv_mfma(x.to(gpu), None, cin, cin, w.to(gpu), None, bias.to(gpu), 1, 1, relu, rows, out_hi=body, f16="plane")
        torch.cuda.synchronize()
        _untouched(f"saturate relu={relu}", buf, body, 0, cout, rows)
        got = body[:rows].float().cpu()
        neg = 0.0 if relu else -65504.0
        assert got[0, 0].item() == 65504.0 and got[0, 1].item() == neg and got[0, 2].item() == 65504.0
        assert got[129, 0].item() == neg and got[129, 1].item() == 65504.0 and got[129, 2].item() == neg
        assert bool(torch.isnan(got[1]).all()), "NaN was laundered"
        keep = torch.ones(rows, dtype=torch.bool); keep[1] = False
        assert bool(torch.isfinite(got[keep]).all()) and not bool(got[2:129].any()) and not bool(got[0, 3:].any())


@pytest.mark.gpu
def test_f16p_refusals_write_nothing(hip_lib, gpu):
    """On the device: the valid launch first, then one field away from it — a lo plane, a bf16-pair residual, the BM256 tiling, out_mode
    0 — each returns MAGNET_E_DIM and writes nothing."""
    import ctypes
    from magnet_amd import lib
    d = _case16(gpu, 64, 64, 9)
    buf, body = _guarded((d["rows"] + EXTRA, 64), gpu, torch.float16)

    def args(**over):
        a = lib.MagnetConvArgs()
        a.in_hi, a.w_hi, a.bias, a.out_hi = d["x16"].data_ptr(), d["w16"].data_ptr(), d["bias"].data_ptr(), body.data_ptr()
        a.rows, a.cin, a.cout_pad, a.taps, a.wp, a.out_mode, a.in_ld = d["rows"], 64, 64, 9, d["wp"], 3, 64
        tiling = over.pop("tiling", 0)
        for k, v in over.items():
            setattr(a, k, v)
        return lib.MagnetConvExArgs(base=a, tiling=tiling)

    f = lib.load().magnet_conv_mfma_f16p
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    with torch.cuda.device(gpu):
        assert f(ctypes.byref(args()), stream) == 0
        torch.cuda.synchronize()
        assert not bool(_sent(body[:d["rows"]]).any())
        body.fill_(float("nan"))
        r = d["r16"].data_ptr()
        for name, over in (("in_lo", dict(in_lo=d["x16"].data_ptr())), ("w_lo", dict(w_lo=d["w16"].data_ptr())),
                           ("add_lo", dict(add_hi=r, add_lo=r)), ("BM256", dict(tiling=lib.TILING_BM256)),
                           ("BM64", dict(tiling=lib.TILING_BM64)), ("out_mode 0", dict(out_mode=0, out_lo=body.data_ptr())),
                           ("addend", dict(addend=d["c"]["addend"].data_ptr())), ("cout_pad 16", dict(cout_pad=16))):
            assert f(ctypes.byref(args(**over)), stream) == lib.E_DIM, name
        torch.cuda.synchronize()
    assert bool(_sent(buf).all())
