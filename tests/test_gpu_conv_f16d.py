"""magnet_conv_mfma_f16d and magnet_conv_mfma_f16d_splitk: the D-Net decoder's plain layers on the single-plane fp16 format ("plane to
plane, wide": any cout_pad % 128 == 0, LeakyReLU, fp16 / fp32 / split-bf16 output), one direct launch per case.

Built like tests/test_gpu_conv_f16p.py, whose helpers (and those of tests/test_gpu_conv_fwd.py, tests/conv_fwd_ref.py) are imported, not
copied: NaN guard bands and sentinel checks around every output, heavy-tailed inputs, every output channel compared.

Shape: N = 2, h = 9, w = 13 on a border of 1 = 2 x 11 x 15 = 330 rows: three 128-row tiles, the last ragged, the image boundary (row 165)
inside the second tile.  The tile count the library reports is asserted in every case.  cout_pad 128 and 256: with two channel blocks
a wrong weight, bias or output offset in blockIdx.y shows.  cin 64 (2 chunks), 160 (5 chunks) and 128 read as channels [64, 192) of a
320-wide plane whose other channels hold data.

Bound (derived, not measured).  The reference is the fp64 convolution of exactly the fp16 planes passed in, so every product x w is
exact in the fp32 accumulator (11 x 11 significant bits).  What is left: K = taps * cin accumulator roundings, the bias addition and
the LeakyReLU product, inside L = K + 5 (tests/test_gpu_conv_f16p.py's K + 4 has the residual's addition where this form has none; the
extra unit here is the LeakyReLU product x * s, one rounding of a value of magnitude <= |x|):
    fp32 output      |out - ref| <= gamma(K + 5) (|x| conv |w| + |bias|)
    fp16 plane       + one fp16 rounding of the result: 2^-11 |ref| where |ref| >= 2^-14, else 2^-25
    split bf16       + the split's dropped part, 2^-16 |v| of the fp32 result v, |v| <= |ref| + the fp32 bound
ReLU and LeakyReLU with slope in (0, 1] are 1-Lipschitz and map 0 to 0: the bound carries through.
Measured worst |error| / bound on MI355X (profiles/dnet_precision/NOTES.md): 0.054 fp32, 0.976 fp16 plane, 0.375 split bf16.

Split-K (S = 2 at cin 160: chunks 2 + 3; S = 3 at cin 224: chunks 2 + 2 + 3, both uneven): no tolerance at all.  Each partial in the
workspace equals the plain entry point's fp32 output on that channel range bit for bit, and the reduced output equals the torch
restatement ((p0 + p1) + p2) + bias, activation, border zeros, output conversion — single IEEE fp32 operations on both sides.  The
limits are magnet_conv_mfma_splitk's, so S = 3 at cin 160 (5 chunks: one split would get a single chunk, below
MAGNET_SPLITK_MIN_CHUNKS) is refused here as it is there; the three-way split therefore runs at cin 224.
"""
import ctypes

import pytest
import torch

from magnet_amd import lib
from magnet_amd.planes import split_bf16, to_f16_sat
from tests import conv_fwd_ref as C
from tests.test_gpu_conv_f16p import _f16_bound, _sent, _untouched
from tests.test_gpu_conv_fwd import EXTRA, _CACHE, _case, _g, _guarded

pytestmark = pytest.mark.gpu

N, H, W, PAD = 2, 9, 13, 1
SLOPE = 0.01
ACTS = [("none", False, None), ("relu", True, None), ("leaky", False, SLOPE)]
WORST = {}


def _case16d(gpu, cin, cout, taps, in_slice=False):
    """fp16 planes of test_gpu_conv_fwd._case at this file's grid and the fp64 pieces of the reference, built once, never modified."""
    key = ("f16d", cin, cout, taps, in_slice)
    if key in _CACHE:
        return _CACHE[key]
    c = _case(gpu, N, H, W, PAD, cin, cout, taps, 1)
    x16 = to_f16_sat(c["hi"].float() + c["lo"].float())
    if in_slice:
        buf = to_f16_sat(torch.randn((c["rows"], 320), generator=_g(91)).to(gpu))
        buf[:, 64:64 + cin] = x16
        x16, in_ld, keep = buf[:, 64:64 + cin], 320, buf
    else:
        x16 = x16.contiguous()
        in_ld, keep = cin, x16
    w16 = to_f16_sat(c["wh"].float() + c["wl"].float()).contiguous()
    K = taps * cin
    conv, b0 = C.conv_ref(x16.double(), w16.double(), taps, c["wp"], c["rows"], 1)
    mag = b0 / (1.01 * C.LOLO + 1.02 * C.gamma_l(3 * K + 2))                           # conv_ref's |x| conv |w|
    d = dict(c=c, x16=x16, in_ld=in_ld, w16=w16, cin=cin, cout=cout, taps=taps, rows=c["rows"], wp=c["wp"], hp=c["hp"], bias=c["bias"],
             inner=c["inner"], conv=conv, mag=mag, K=K, _keep=keep)
    assert d["rows"] == 330
    _CACHE[key] = d
    return d


def _ref(d, relu, leaky):
    """(ref, bound) of the fp32 result: see the module docstring."""
    bias = d["bias"].double()[:d["cout"]]
    ref = d["conv"] + bias
    bound = C.gamma_l(d["K"] + 5) * (d["mag"] + bias.abs())
    if relu:
        ref = ref.clamp_min(0.0)
    elif leaky is not None:
        ref = torch.where(ref < 0, ref * C.f32(leaky), ref)
    return ref, bound


def _launch(d, relu, leaky, **kw):
    n = lib.conv_mfma(d["x16"], None, d["in_ld"], d["cin"], d["w16"], None, d["bias"], d["taps"], d["wp"], relu, d["rows"], leaky=leaky,
                      f16="wide", **kw)
    torch.cuda.synchronize()
    return n


def _note(kind, worst):
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    print(f"[conv f16d] worst |error| / bound so far, {kind}: {WORST[kind]:.4f}")


CASES = [(f"t{t}-{'slice128' if sl else ci}x{co}", ci, co, t, sl) for t in (9, 1) for ci, sl in ((64, False), (160, False), (128, True))
         for co in (128, 256)]
PARAMS = dict(argnames="cin,cout,taps,in_slice", argvalues=[t[1:] for t in CASES], ids=[t[0] for t in CASES])


@pytest.mark.parametrize("act,relu,leaky", ACTS, ids=[a[0] for a in ACTS])
@pytest.mark.parametrize(**PARAMS)
def test_f16d_plane_output(hip_lib, gpu, request, cin, cout, taps, in_slice, act, relu, leaky):
    """fp16 plane in, fp16 plane out (out_mode 3) with the zero border: the decoder's up*.mid."""
    name = request.node.callspec.id
    d = _case16d(gpu, cin, cout, taps, in_slice)
    ref, bound = _ref(d, relu, leaky)
    ref, bound, _ = C.border_and_repad(ref, _f16_bound(ref, bound), N, d["hp"], d["wp"], PAD, 0)
    buf, body = _guarded((d["rows"] + EXTRA, cout), gpu, torch.float16)
    tiles = _launch(d, relu, leaky, out_hi=body, border=(d["hp"], PAD))
    assert tiles == 3, f"{name}: {tiles} tiles: not a 128-row instance"
    _untouched(name, buf, body, 0, cout, d["rows"])
    got = body[:d["rows"]]
    worst = C.check(name, got, ref, bound)
    assert bool((got[~d["inner"]].contiguous().view(torch.int16) == 0).all()), f"{name}: a border position is not +0"
    _note("fp16 plane", worst)


@pytest.mark.parametrize("act,relu,leaky", ACTS, ids=[a[0] for a in ACTS])
@pytest.mark.parametrize(**PARAMS)
def test_f16d_fp32_repad_output(hip_lib, gpu, request, cin, cout, taps, in_slice, act, relu, leaky):
    """fp32 output with repad = 1 (out_mode 1): the compact hand-over to the bilinear upsampling (d0, up*.out)."""
    name = request.node.callspec.id
    d = _case16d(gpu, cin, cout, taps, in_slice)
    ref, bound = _ref(d, relu, leaky)
    ref, bound, written = C.border_and_repad(ref, bound, N, d["hp"], d["wp"], PAD, 1)
    assert ref.shape[0] == N * H * W and bool(written.all())
    buf, body = _guarded((ref.shape[0] + EXTRA, cout), gpu)
    tiles = _launch(d, relu, leaky, out_f32=body, border=(d["hp"], PAD), repad=1)
    assert tiles == 3
    _untouched(name, buf, body, 0, cout, ref.shape[0])
    _note("fp32 repad", C.check(name, body[:ref.shape[0]], ref, bound))


@pytest.mark.parametrize("act,relu,leaky", ACTS, ids=[a[0] for a in ACTS])
@pytest.mark.parametrize(**PARAMS)
def test_f16d_split_bf16_slice_output(hip_lib, gpu, request, cin, cout, taps, in_slice, act, relu, leaky):
    """split-bf16 planes (out_mode 0) into channels [64, 64 + cout) of a wider buffer, zero border: x_feat into G-Net's input buffer."""
    name = request.node.callspec.id
    d = _case16d(gpu, cin, cout, taps, in_slice)
    ref, bound = _ref(d, relu, leaky)
    bound = bound + 2.0 ** -16 * (ref.abs() + bound)
    ref, bound, _ = C.border_and_repad(ref, bound, N, d["hp"], d["wp"], PAD, 0)
    ctot, o0 = cout + 128, 64
    bh, hi = _guarded((d["rows"] + EXTRA, ctot), gpu, torch.bfloat16)
    bl, lo = _guarded((d["rows"] + EXTRA, ctot), gpu, torch.bfloat16)
    tiles = _launch(d, relu, leaky, out_hi=hi[:, o0:o0 + cout], out_lo=lo[:, o0:o0 + cout], out_ld=ctot, border=(d["hp"], PAD))
    assert tiles == 3
    for b, body in ((bh, hi), (bl, lo)):
        _untouched(name, b, body, o0, o0 + cout, d["rows"])
    got = hi[:d["rows"], o0:o0 + cout].double() + lo[:d["rows"], o0:o0 + cout].double()
    worst = C.check(name, got, ref, bound)
    for body in (hi, lo):
        assert bool((body[:d["rows"], o0:o0 + cout][~d["inner"]].contiguous().view(torch.int16) == 0).all()), f"{name}: border not +0"
    _note("split bf16 slice", worst)


@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
def test_f16d_store_saturates(hip_lib, gpu, act):
    """A row of 32 x 65504 against weights +1 / -1 / +2^-5 sums to +-2 096 128 and 65504 in fp32; the fp16 store clamps the first two to
    +-65504 (never Inf) and keeps the third; with ReLU the negative one is +0, with LeakyReLU it is f16(-2 096 128 x 0.01).  The second
    channel block (cout_pad 256) carries the same weights at channels 128 .. 130."""
    rows, cin, cout = 130, 32, 256                                                  # two tiles, the second ragged
    x = torch.zeros((rows, cin), dtype=torch.float16)
    x[0] = 65504.0
    x[129] = -65504.0
    w = torch.zeros((1, cout, cin), dtype=torch.float16)
    for c0 in (0, 128):
        w[0, c0], w[0, c0 + 1], w[0, c0 + 2] = 1.0, -1.0, 2.0 ** -5
    buf, body = _guarded((rows + EXTRA, cout), gpu, torch.float16)
    lib.conv_mfma(x.to(gpu), None, cin, cin, w.to(gpu), None, torch.zeros(cout, device=gpu), 1, 1, act == "relu", rows, out_hi=body,
                  leaky=SLOPE if act == "leaky" else None, f16="wide")
    torch.cuda.synchronize()
    _untouched(f"saturate {act}", buf, body, 0, cout, rows)
    got = body[:rows].float().cpu()
    s = torch.tensor(-2096128.0) * torch.tensor(SLOPE, dtype=torch.float32)
    neg = {"none": -65504.0, "relu": 0.0, "leaky": float(to_f16_sat(s))}[act]
    for c0 in (0, 128):
        assert got[0, c0].item() == 65504.0 and got[0, c0 + 1].item() == neg and got[0, c0 + 2].item() == 65504.0
        assert got[129, c0].item() == neg and got[129, c0 + 1].item() == 65504.0
    assert bool(torch.isfinite(got).all()) and not bool(got[1:129].any())


def test_f16d_nan_passes_through(hip_lib, gpu):
    """A NaN operand makes its whole output row NaN (0 x NaN = NaN in the matrix instruction); the fp16 store writes NaN through, under
    every activation, and no other row is touched by it."""
    rows, cin, cout = 130, 32, 128
    x = torch.ones((rows, cin), dtype=torch.float16)
    x[1, 3] = float("nan")
    w = torch.full((1, cout, cin), 2.0 ** -5, dtype=torch.float16)
    for relu, leaky in ((False, None), (True, None), (False, SLOPE)):
        buf, body = _guarded((rows + EXTRA, cout), gpu, torch.float16)
        lib.conv_mfma(x.to(gpu), None, cin, cin, w.to(gpu), None, torch.zeros(cout, device=gpu), 1, 1, relu, rows, out_hi=body, leaky=leaky,
                      f16="wide")
        torch.cuda.synchronize()
        _untouched("nan", buf, body, 0, cout, rows)
        got = body[:rows].float().cpu()
        assert bool(torch.isnan(got[1]).all()), "NaN was laundered"
        keep = torch.ones(rows, dtype=torch.bool); keep[1] = False
        assert bool((got[keep] == 1.0).all())


def _ex_args(d, body, **over):
    a = lib.MagnetConvArgs()
    a.in_hi, a.w_hi, a.bias, a.out_hi = d["x16"].data_ptr(), d["w16"].data_ptr(), d["bias"].data_ptr(), body.data_ptr()
    a.rows, a.cin, a.cout_pad, a.taps, a.wp, a.out_mode, a.in_ld = d["rows"], d["cin"], d["cout"], d["taps"], d["wp"], 3, d["in_ld"]
    tiling = over.pop("tiling", 0)
    for k, v in over.items():
        setattr(a, k, v)
    return lib.MagnetConvExArgs(base=a, tiling=tiling)


def test_f16d_refusals_write_nothing(hip_lib, gpu):
    """The valid launch first, then one field away from it: each returns MAGNET_E_DIM and writes nothing."""
    d = _case16d(gpu, 64, 128, 9)
    buf, body = _guarded((d["rows"] + EXTRA, 128), gpu, torch.float16)
    f = lib.load().magnet_conv_mfma_f16d
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    x, wt, bias, r = d["x16"].data_ptr(), d["w16"].data_ptr(), d["bias"].data_ptr(), d["c"]["addend"].data_ptr()
    with torch.cuda.device(gpu):
        assert f(ctypes.byref(_ex_args(d, body)), stream) == 0
        torch.cuda.synchronize()
        assert not bool(_sent(body[:d["rows"]]).any())
        body.fill_(float("nan"))
        for name, over in (("in_lo", dict(in_lo=x)), ("residual plane", dict(add_hi=r)), ("residual pair", dict(add_hi=r, add_lo=r)),
                           ("addend", dict(addend=r)),
                           ("fused tail", dict(tail_w_hi=wt, tail_w_lo=wt, tail_bias=bias, tail_cout_pad=16, out_mode=1, out_f32=body.data_ptr())),
                           ("BM64", dict(tiling=lib.TILING_BM64)), ("BM256", dict(tiling=lib.TILING_BM256)),
                           ("cout_pad 64", dict(cout_pad=64)), ("out_mode 2", dict(out_mode=2)), ("w_lo", dict(w_lo=wt)),
                           ("taps 4", dict(taps=4)), ("dil 2", dict(dil=2))):
            assert f(ctypes.byref(_ex_args(d, body, **over)), stream) == lib.E_DIM, name
        torch.cuda.synchronize()
    assert bool(_sent(buf).all())


# ---- split-K ----------------------------------------------------------------------------------------------------------------------
SK_CASES = [(9, 160, 2), (1, 160, 2), (9, 224, 3), (1, 224, 3)]
SK_COUT = 256
SK_SENT = 7.0


def _ranges(cin, S):
    n = cin // 32
    return [(z * n // S * 32, (z + 1) * n // S * 32) for z in range(S)]


def _sk_setup(gpu, taps, cin, S):
    """The case, the plain entry point's fp32 output per channel range and their fixed-order fp32 sum + bias, computed once."""
    key = ("f16d-sk", taps, cin, S)
    if key in _CACHE:
        return _CACHE[key]
    d = _case16d(gpu, cin, SK_COUT, taps)
    zero = torch.zeros(SK_COUT, device=gpu)
    parts = []
    for c0, c1 in _ranges(cin, S):
        o = torch.full((d["rows"], SK_COUT), SK_SENT, device=gpu)
        lib.conv_mfma(d["x16"][:, c0:], None, cin, c1 - c0, d["w16"][:, :, c0:c1].contiguous(), None, zero, taps, d["wp"], False, d["rows"],
                      out_f32=o, f16="wide")
        parts.append(o)
    acc = parts[0].clone()
    for p in parts[1:]:
        acc = acc + p                                                   # fp32, ascending s
    _CACHE[key] = dict(d=d, parts=parts, pre=acc + d["bias"])
    assert len({c1 - c0 for c0, c1 in _ranges(cin, S)}) > 1              # uneven ranges
    return _CACHE[key]


def _sk_expected(k, act):
    pre, d = k["pre"], k["d"]
    if act == "relu":
        v = pre.clamp_min(0.0)
    elif act == "leaky":
        v = torch.where(pre < 0, pre * torch.tensor(SLOPE, dtype=torch.float32, device=pre.device), pre)
    else:
        v = pre
    return torch.where(d["inner"][:, None], v, torch.zeros_like(v))     # border positions: +0


def _sk_run(k, taps, cin, S, work, act="leaky", **kw):
    d = k["d"]
    return lib.conv_mfma(d["x16"], None, cin, cin, d["w16"], None, d["bias"], taps, d["wp"], act == "relu", d["rows"],
                         leaky=SLOPE if act == "leaky" else None, border=(d["hp"], PAD), f16="wide", split_k=S, work=work, **kw)


def _work(gpu, S, rows):
    full = torch.full((S * rows * SK_COUT + 4096,), SK_SENT, device=gpu)
    return full, full[:S * rows * SK_COUT]


@pytest.mark.parametrize("taps,cin,S", SK_CASES)
def test_f16d_splitk_partials_are_the_plain_launch_on_each_range(hip_lib, gpu, taps, cin, S):
    k = _sk_setup(gpu, taps, cin, S)
    rows = k["d"]["rows"]
    full, work = _work(gpu, S, rows)
    out = torch.full((rows, SK_COUT), SK_SENT, device=gpu)
    assert _sk_run(k, taps, cin, S, work, out_f32=out) == 3
    got = work.reshape(S, rows, SK_COUT)
    for z in range(S):
        assert torch.equal(got[z], k["parts"][z]), f"partial {z} of {S} differs from the plain launch on its channel range"
    assert bool((full[S * rows * SK_COUT:] == SK_SENT).all())             # the ragged tile wrote nothing behind the workspace


@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
@pytest.mark.parametrize("form", ["f16", "f32-repad", "bf16-slice"])
@pytest.mark.parametrize("taps,cin,S", SK_CASES)
def test_f16d_splitk_output_is_the_fixed_order_sum_bitwise(hip_lib, gpu, taps, cin, S, form, act):
    k = _sk_setup(gpu, taps, cin, S)
    d = k["d"]
    rows = d["rows"]
    _, work = _work(gpu, S, rows)
    exp = _sk_expected(k, act)
    if act == "leaky":
        assert float((k["pre"] < 0).float().mean()) > 0.2                 # the negative branch is exercised
    if form == "f16":
        buf, body = _guarded((rows + EXTRA, SK_COUT), gpu, torch.float16)
        _sk_run(k, taps, cin, S, work, act, out_hi=body)
        torch.cuda.synchronize()
        _untouched("splitk f16", buf, body, 0, SK_COUT, rows)
        assert torch.equal(body[:rows].view(torch.int16), to_f16_sat(exp).view(torch.int16))
    elif form == "f32-repad":
        n = N * H * W
        buf, body = _guarded((n + EXTRA, SK_COUT), gpu)
        _sk_run(k, taps, cin, S, work, act, out_f32=body, repad=1)
        torch.cuda.synchronize()
        _untouched("splitk f32", buf, body, 0, SK_COUT, n)
        assert torch.equal(body[:n], exp[d["inner"]])
    else:
        ctot, o0 = SK_COUT + 128, 64
        bh, hi = _guarded((rows + EXTRA, ctot), gpu, torch.bfloat16)
        bl, lo = _guarded((rows + EXTRA, ctot), gpu, torch.bfloat16)
        _sk_run(k, taps, cin, S, work, act, out_hi=hi[:, o0:o0 + SK_COUT], out_lo=lo[:, o0:o0 + SK_COUT], out_ld=ctot)
        torch.cuda.synchronize()
        eh, el = split_bf16(exp)
        for b, body, e in ((bh, hi, eh), (bl, lo, el)):
            _untouched("splitk bf16", b, body, o0, o0 + SK_COUT, rows)
            assert torch.equal(body[:rows, o0:o0 + SK_COUT].contiguous().view(torch.int16), e.view(torch.int16))


def test_f16d_splitk_refusals_write_nothing(hip_lib, gpu):
    taps, cin, S = 9, 160, 2
    k = _sk_setup(gpu, taps, cin, S)
    d = k["d"]
    rows = d["rows"]
    full, work = _work(gpu, S, rows)
    out = torch.full((rows, SK_COUT), SK_SENT, device=gpu)
    _sk_run(k, taps, cin, S, work, out_f32=out)                           # the valid launch
    assert torch.equal(out, _sk_expected(k, "leaky"))
    full.fill_(SK_SENT); out.fill_(SK_SENT)

    def refused(code, S_=S, work_=work, **kw):
        kw.setdefault("out_f32", out)
        with pytest.raises(lib.MagnetError) as e:
            _sk_run(k, taps, cin, S_, work_, **kw)
        assert e.value.code == code, e.value
    refused(lib.E_DIM, S_=9)
    refused(lib.E_DIM, S_=1)
    refused(lib.E_DIM, S_=3)                                              # 5 chunks over 3 splits: the limit of magnet_conv_mfma_splitk
    refused(lib.E_DIM, work_=work[:-4])                                   # too small
    refused(lib.E_ALIGN, work_=full[1:1 + work.numel()])                  # misaligned
    refused(lib.E_DIM, tiling=lib.TILING_BM64)
    refused(lib.E_DIM, tiling=lib.TILING_BM256)
    # a NULL workspace, through the C entry point itself
    body = torch.full((rows, SK_COUT), float("nan"), dtype=torch.float16, device=gpu)
    f = lib.load().magnet_conv_mfma_f16d_splitk
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    with torch.cuda.device(gpu):
        assert f(ctypes.byref(_ex_args(d, body)), S, None, work.numel() * 4, stream) == lib.E_NULL
        assert f(ctypes.byref(_ex_args(d, body, in_lo=d["x16"].data_ptr())), S, work.data_ptr(), work.numel() * 4, stream) == lib.E_DIM
        assert f(ctypes.byref(_ex_args(d, body, out_mode=2)), S, work.data_ptr(), work.numel() * 4, stream) == lib.E_DIM
    torch.cuda.synchronize()
    assert bool((full == SK_SENT).all()) and bool((out == SK_SENT).all()) and bool(_sent(body).all())
