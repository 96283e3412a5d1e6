"""The encoder's fp16 single-plane mode on the GPU (EncoderMFMA(precision="fp16"); magnet_enc_stem_f16, magnet_dwconv_cl_f16,
magnet_se_scale_f16, magnet_conv_mfma_f16e): every launch on its own, pointwise against the fp64 restatements and derived bounds of
tests/encoder_f16_ref.py; bit equality with the routes whose kernel instances magnet_conv_mfma_f16e shares; its refusals on the device;
then the whole encoder and the whole D-Net against the CPU emulation of the format (tests/encoder_f16_ref.emulate): per tap
err_hip <= 2 err_emulated, both taken against the plain fp64 forward.  The default path stays what it was, to the bit.

The mode is outside the project's 1e-4 contract.  Measured on one MI355X (largest |difference from fp64| as a fraction of the tap's
largest magnitude, HIP / emulated): profiles/encoder_precision/NOTES.md."""
import ctypes
import functools

import pytest
import torch

from tests import conv_fwd_ref as C
from tests import encoder_f16_ref as F
from tests import encoder_ref as R
from tests.test_gpu_encoder import _border_untouched, _encoder_case, _guards_untouched, _rand

pytestmark = pytest.mark.gpu


def _nan_plane(rows, c, gpu):
    return R.guarded((rows, c), gpu, torch.float16)


def _img(plane, N, h, w):
    """The interior of an fp16 plane (rows, c) as fp64 NCHW."""
    return R.interior(plane.cpu().double(), N, h, w)


# ---- depthwise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(9, 13), (18, 26), (37, 70)])
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("C_,c_pad", [(48, 64), (144, 160)])
def test_dwconv_f16_against_fp64(hip_lib, gpu, C_, c_pad, k, stride, h, w):
    from magnet_amd import lib
    N = 2
    x = F.f16_exact(_rand((N, C_, h, w), 11 * h + k + stride, 1.5))
    xp, x64 = F.to_plane(x, c_pad)
    wgt = torch.zeros((k * k, c_pad)); wgt[:, :C_] = _rand((k * k, C_), 5 + k, 0.4)
    bias = torch.zeros(c_pad); bias[:C_] = _rand((C_,), 6 + k, 0.3)
    (pt, _), (pl, _) = R.same_pad(h, k, stride), R.same_pad(w, k, stride)
    ho, wo = -(-h // stride), -(-w // stride)
    bo, out = _nan_plane(N * (ho + 2) * (wo + 2), c_pad, gpu)
    n_part = lib.dwconv_parts(ho, wo)
    bp, part = R.guarded((N, n_part, c_pad), gpu)
    assert lib.dwconv_cl_f16(xp.to(gpu), c_pad, N, h, w, c_pad, wgt.to(gpu), bias.to(gpu), k, stride, pt, pl, out, c_pad, part) == n_part
    torch.cuda.synchronize()
    name = f"dwconv f16 k{k} s{stride} {h}x{w} C{C_}"
    _guards_untouched(name, bo, bp)
    _border_untouched(name, out, N, ho, wo)
    ref, b32, bpl = F.dwconv_ref(R.interior(x64, N, h, w), wgt, bias, k, stride, pt, pl)
    got = _img(out, N, ho, wo)
    worst = R.check(name, got, ref, bpl)
    assert bool((got[:, C_:] == 0).all()), f"{name}: pad lanes not zero"
    pref, pb = R.dw_partials_ref(ref, b32)                            # from the fp32 values before the store: today's bound
    wp = R.check(name + " partials", part.cpu().double(), pref, pb)
    print(f"{name}: outputs {worst:.3f}, partials {wp:.3f} of the bound")


# ---- scale and stem ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [48, 1056, 3072])
def test_se_scale_f16_against_fp64(hip_lib, gpu, C_):
    from magnet_amd import lib
    N, h, w = 2, 5, 7
    c_pad = (C_ + 31) // 32 * 32
    x = F.f16_exact(_rand((N, C_, h, w), C_, 1.0))
    xp, x64 = F.to_plane(x, c_pad)
    gate = torch.zeros((N, c_pad)); gate[:, :C_] = torch.sigmoid(_rand((N, C_), C_ + 1, 2.0))
    rows = N * (h + 2) * (w + 2)
    bo, out = _nan_plane(rows, c_pad, gpu)
    src = xp.to(gpu)
    lib.se_scale_f16(src, c_pad, gate.to(gpu), N, h, w, c_pad, out, c_pad)
    inp = src.clone()
    lib.se_scale_f16(inp, c_pad, gate.to(gpu), N, h, w, c_pad, inp, c_pad)
    torch.cuda.synchronize()
    _guards_untouched("se_scale f16", bo)
    _border_untouched("se_scale f16", out, N, h, w)
    ref, b = F.se_scale_ref(R.interior(x64, N, h, w), gate)
    ws = R.check(f"se_scale f16 C{C_}", _img(out, N, h, w), ref, b)
    assert torch.equal(_img(inp, N, h, w), _img(out, N, h, w)), "in place differs"
    g = inp.reshape(N, h + 2, w + 2, -1)
    assert bool((g[:, 0] == 0).all() and (g[:, -1] == 0).all() and (g[:, :, 0] == 0).all() and (g[:, :, -1] == 0).all())
    assert float((gate[0, :C_] - gate[1, :C_]).abs().max()) > 1e-3         # the two images' gates differ: a wrong image index shows
    print(f"se_scale f16 C{C_}: {ws:.3f} of the bound")


@pytest.mark.parametrize("shape", [(2, 3, 72, 104), (1, 3, 71, 103)])
def test_stem_f16_against_fp64(hip_lib, gpu, shape):
    from magnet_amd import lib
    N, _, H, W = shape
    img = torch.rand(shape, generator=torch.Generator().manual_seed(H))
    wgt, bias = _rand((48, 27), 1, 0.3), _rand((48,), 2, 0.2)
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    bo, out = _nan_plane(N * (H2 + 2) * (W2 + 2), 64, gpu)
    lib.enc_stem_f16(img.to(gpu), wgt.to(gpu), bias.to(gpu), out)
    torch.cuda.synchronize()
    _guards_untouched("stem f16", bo)
    _border_untouched("stem f16", out, N, H2, W2)
    got = _img(out, N, H2, W2)
    ref, b = F.stem_ref(img, wgt, bias)
    worst = R.check(f"stem f16 {H}x{W}", got[:, :48], ref, b)
    assert bool((got[:, 48:] == 0).all()), "stem f16: channels 48..63 not zero"
    print(f"stem f16 {H}x{W}: {worst:.3f} of the bound")


# ---- magnet_conv_mfma_f16e -----------------------------------------------------------------------------------------------------------
N_, H_, W_ = 2, 7, 9
HP, WP = H_ + 2, W_ + 2
ROWS = N_ * HP * WP                                                   # 198 rows: two 128-row tiles, the second partial


@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout):
    """fp16-representable operands of one 1x1 layer on the (2, 7, 9) grid: planes on the CPU with their fp64 images (made once)."""
    x = F.f16_exact(_rand((N_, cin, H_, W_), cin, 1.0))
    xp, x64 = F.to_plane(x, cin)
    w16 = _rand((1, cout, cin), cout, (2.0 / cin) ** 0.5).to(torch.float16)
    bias = _rand((cout,), cout + 1, 0.2)
    rp, r64 = F.to_plane(F.f16_exact(_rand((N_, cout, H_, W_), cout + 2, 1.0)), cout)
    return dict(xp=xp, x64=x64, w16=w16, w64=w16.double(), bias=bias, rp=rp, r64=r64, cin=cin, cout=cout)


def _conv_launch(c, gpu, res, silu, route="enc", w=None, bias=None, **kw):
    from magnet_amd import lib
    w = c["w16"] if w is None else w
    bias = c["bias"] if bias is None else bias
    n = lib.conv_mfma(c["xp"].to(gpu), None, c["cin"], c["cin"], w.to(gpu), None, bias.to(gpu), 1, WP, False, ROWS,
                      add=(c["rp"].to(gpu), None, c["cout"]) if res else None, f16=route, **({"silu": True} if silu else {}), **kw)
    torch.cuda.synchronize()
    return n


@pytest.mark.parametrize("silu", [False, True], ids=["base", "silu"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("cin,cout", [(64, 32), (160, 64), (512, 2048)])
def test_conv_f16e_against_fp64(hip_lib, gpu, cin, cout, res, silu):
    c = _conv_case(cin, cout)
    name = f"conv f16e {cin}->{cout} res={res} silu={silu}"
    # out_mode 3: one fp16 plane, zero border
    ref, b = F.conv_ref_f16(c["x64"], c["w64"], c["bias"], WP, ROWS, res=c["r64"] if res else None, silu=silu, plane=True)
    eref, eb, _ = C.border_and_repad(ref, b, N_, HP, WP, 1, 0)
    bo, out = _nan_plane(ROWS, cout, gpu)
    tiles = _conv_launch(c, gpu, res, silu, out_hi=out, border=(HP, 1))
    assert tiles == -(-ROWS // 128)
    _guards_untouched(name, bo)
    w3 = C.check(name + " fp16", out.cpu(), eref, eb)
    inner = C.interior(N_, HP, WP, 1)
    assert bool((out.cpu()[~inner].view(torch.int16) == 0).all()), f"{name}: a border position is not +0"
    # out_mode 1: fp32, interior rows re-addressed to the grid without border (repad = 1)
    ref, b = F.conv_ref_f16(c["x64"], c["w64"], c["bias"], WP, ROWS, res=c["r64"] if res else None, silu=silu, plane=False)
    eref, eb, written = C.border_and_repad(ref, b, N_, HP, WP, 1, 1)
    bf, o32 = R.guarded((N_ * H_ * W_, cout), gpu)
    _conv_launch(c, gpu, res, silu, out_f32=o32, border=(HP, 1), repad=1)
    _guards_untouched(name, bf)
    assert bool(written.all()) and not bool(torch.isnan(o32).any())
    w1 = C.check(name + " fp32", o32.cpu(), eref.reshape(-1, cout), eb.reshape(-1, cout))
    print(f"{name}: fp16 plane {w3:.3f}, fp32 {w1:.3f} of the bound")


def test_conv_f16e_slice_pair_fills_a_160_wide_buffer(hip_lib, gpu):
    """Stage 1's expand layer: 144 outputs as 128 + 32 channel slices of a 160-wide plane, each launch leaving the other's channels alone."""
    cin, cout, width = 32, 144, 160
    x = F.f16_exact(_rand((N_, cin, H_, W_), 7, 1.0))
    xp, x64 = F.to_plane(x, cin)
    w16 = torch.zeros((1, width, cin), dtype=torch.float16); w16[:, :cout] = _rand((1, cout, cin), 8, 0.25).to(torch.float16)
    bias = torch.zeros(width); bias[:cout] = _rand((cout,), 9, 0.2)
    c = dict(xp=xp, cin=cin, cout=width, w16=w16, bias=bias)
    bo, out = _nan_plane(ROWS, width, gpu)
    _conv_launch(c, gpu, False, True, w=w16[:, :128].contiguous(), bias=bias[:128].contiguous(), out_hi=out[:, :128], out_ld=width, border=(HP, 1))
    first = out.clone()
    assert bool(torch.isnan(first[:, 128:]).all()) and not bool(torch.isnan(first[:, :128]).any()), "the 128-wide launch wrote outside its slice"
    _conv_launch(c, gpu, False, True, w=w16[:, 128:].contiguous(), bias=bias[128:].contiguous(), out_hi=out[:, 128:], out_ld=width, border=(HP, 1))
    _guards_untouched("slice pair", bo)
    assert torch.equal(out[:, :128], first[:, :128]), "the 32-wide launch wrote outside its slice"
    ref, b = F.conv_ref_f16(x64, w16.double(), bias, WP, ROWS, silu=True, plane=True)
    eref, eb, _ = C.border_and_repad(ref, b, N_, HP, WP, 1, 0)
    worst = C.check("slice pair", out.cpu(), eref, eb)
    assert bool((out.cpu()[:, cout:] == 0).all()), "pad lanes not zero"
    print(f"conv f16e 128 + 32 slices: {worst:.3f} of the bound")


@pytest.mark.parametrize("cin,cout", [(64, 32), (160, 64), (512, 2048)])
def test_conv_f16e_equals_the_routes_it_shares_instances_with(hip_lib, gpu, cin, cout):
    c = _conv_case(cin, cout)
    for res in ((False, True) if cout in (32, 64) else (False,)):
        route = "plane" if cout in (32, 64) else "wide"
        for mode in ("plane", "fp32"):
            outs = []
            for r in ("enc", route):
                if mode == "plane":
                    _, o = _nan_plane(ROWS, cout, gpu)
                    _conv_launch(c, gpu, res, False, route=r, out_hi=o, border=(HP, 1))
                else:
                    _, o = R.guarded((ROWS, cout), gpu)
                    _conv_launch(c, gpu, res, False, route=r, out_f32=o)
                outs.append(o)
            assert not bool(torch.isnan(outs[0].float()).any())
            same = torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) if mode == "plane" else torch.equal(outs[0], outs[1])
            assert same, f"{cin}->{cout} res={res} {mode}: magnet_conv_mfma_f16e differs from f16='{route}'"


def test_conv_f16e_refusals_on_the_device(hip_lib, gpu):
    """The valid launch first; then one field away from it: MAGNET_E_DIM, and the NaN-prefilled output stays untouched."""
    from magnet_amd import lib
    c = _conv_case(64, 32)
    L = hip_lib
    keep = [c["xp"].to(gpu), c["w16"].to(gpu), c["bias"].to(gpu), c["rp"].to(gpu), torch.zeros(4096, dtype=torch.float16, device=gpu)]
    bo, out = _nan_plane(ROWS, 128, gpu)                               # wide enough for every cout_pad tried below

    def args(**kw):
        x = lib.MagnetConvExArgs()
        b = x.base
        b.in_hi, b.w_hi, b.bias, b.out_hi, b.add_hi = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), out.data_ptr(), keep[3].data_ptr()
        b.rows, b.cin, b.cout_pad, b.taps, b.wp, b.out_mode = ROWS, 64, 32, 1, WP, 3
        b.in_ld, b.out_ld, b.add_ld, b.border_hp, b.border_pad = 64, 128, 32, HP, 1
        x.act = lib.ACT_SILU
        for k, v in kw.items():
            setattr(b if hasattr(b, k) else x, k, v)
        return x

    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    with torch.cuda.device(gpu):
        assert L.magnet_conv_mfma_f16e(ctypes.byref(args()), stream) == 0, L.magnet_last_error().decode()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out[:, :32]).any()) and bool(torch.isnan(out[:, 32:]).all())
        out.fill_(float("nan"))
        spare = keep[4].data_ptr()
        for what, kw in (("in_lo", dict(in_lo=spare)), ("add_lo", dict(add_lo=spare)), ("taps 9", dict(taps=9)), ("cout_pad 144", dict(cout_pad=144)),
                         ("relu", dict(relu=1)), ("LeakyReLU", dict(act=lib.ACT_LEAKY_RELU, act_slope=0.1)), ("fused tail", dict(tail_w_hi=spare)),
                         ("BM64", dict(tiling=lib.TILING_BM64))):
            assert L.magnet_conv_mfma_f16e(ctypes.byref(args(**kw)), stream) == lib.E_DIM, (what, L.magnet_last_error().decode())
            assert L.magnet_last_error().decode().startswith("magnet_conv_mfma_f16e:"), what
        torch.cuda.synchronize()
    assert bool(torch.isnan(bo).all()), "a refused call wrote to the output"


# ---- the whole encoder, the whole D-Net ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emulated(H, W):
    """The CPU emulation of the format for _encoder_case(H, W)'s module and images (computed once, never changed)."""
    from magnet_amd.encoder import Encoder
    enc, img, _, _ = _encoder_case(H, W)
    ref = Encoder()
    ref.load_state_dict(enc.state_dict())
    return F.emulate(ref.eval(), img)


def _fp16_encoder(H, W, gpu):
    from magnet_amd.encoder import Encoder
    enc, img, f64, _ = _encoder_case(H, W)
    e16 = Encoder(backend="hip", precision="fp16")
    e16.load_state_dict(enc.state_dict())
    return e16.to(gpu).eval(), img, f64


@pytest.mark.parametrize("H,W", [(72, 104), (64, 96)])
def test_encoder_f16_within_twice_the_emulated_error(hip_lib, gpu, H, W):
    from magnet_amd.encoder import TAPS
    e16, img, f64 = _fp16_encoder(H, W, gpu)
    emu = _emulated(H, W)
    with torch.no_grad():
        got = e16(img.to(gpu))
        one = [e16(img[i:i + 1].to(gpu)) for i in range(2)]
    assert len(got) == 16 and got[0].shape == img.shape and all(got[i] is None for i in range(16) if i not in (0,) + TAPS)
    fails = []
    for i in TAPS:
        top = float(f64[i].abs().max())
        e_hip = float((got[i].cpu().double() - f64[i]).abs().max()) / top
        e_emu = float((emu[i] - f64[i]).abs().max()) / top
        print(f"encoder fp16 {H}x{W} tap [{i}] {tuple(got[i].shape)}: max |x| {top:.3g}; HIP {e_hip:.3g}, emulated {e_emu:.3g} of it (bar 2 x emulated)")
        assert got[i].shape == f64[i].shape and got[i].dtype == torch.float32 and bool(torch.isfinite(got[i]).all())
        if not e_hip <= 2.0 * e_emu:
            fails.append((i, e_hip, e_emu))
        for n in range(2):
            assert torch.equal(one[n][i][0], got[i][n]), f"tap [{i}]: image {n} alone differs from image {n} in the batch"
    assert not fails, f"taps over twice the emulated error (index, HIP, emulated): {fails}"


def test_default_path_is_untouched_by_the_fp16_runner(hip_lib, gpu):
    from magnet_amd.encoder import Encoder, EncoderMFMA, TAPS
    enc, img, _, _ = _encoder_case(64, 96)
    enc = enc.to(gpu)
    named = Encoder(backend="hip", precision="bf16x3")
    named.load_state_dict(enc.state_dict())
    named = named.to(gpu).eval()
    x = img.to(gpu)
    f16 = EncoderMFMA(enc.original_model, precision="fp16")           # a second runner on the SAME module
    with torch.no_grad():
        a, b = enc(x), named(x)
        h = f16(x)
        again = enc(x)
        h2 = f16(x)
    for i in TAPS:
        assert torch.equal(a[i], b[i]), f"tap [{i}]: precision='bf16x3' differs from the default"
        assert torch.equal(a[i], again[i]), f"tap [{i}]: an fp16 run on the same module changed the bf16x3 result"
        assert torch.equal(h[i], h2[i]), f"tap [{i}]: a bf16x3 run on the same module changed the fp16 result"
        assert not torch.equal(a[i], h[i]), f"tap [{i}]: the fp16 result equals the bf16x3 result"


@functools.lru_cache(maxsize=None)
def _dnet_case(gpu):
    """The seeded stand-alone D-Net at 64x96: its state, the torch fp32 output on the GPU, and the fp64 torch decoder on the CPU fed with
    the emulated taps and with the plain fp64 taps (computed once, never changed)."""
    from magnet_amd.dnet import DNET, gaussian_activation, load_seeded_decoder
    from magnet_amd.encoder import Encoder
    from magnet_amd.standin import make_dnet_args
    enc, img, f64, _ = _encoder_case(64, 96)
    ref = DNET(make_dnet_args(), Encoder(), dnet=True)
    ref.d_net.encoder.load_state_dict(enc.state_dict())
    load_seeded_decoder(ref.d_net.decoder, 0)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    ref = ref.to(gpu).eval()
    with torch.no_grad():
        b = ref(img.to(gpu)).cpu()
        dec64 = ref.d_net.decoder.cpu().double()
        emu = gaussian_activation(dec64(_emulated(64, 96)), magnet=False)
        plain = gaussian_activation(dec64(f64), magnet=False)
    return state, img, b, emu, plain


@pytest.mark.parametrize("decoder_precision", ["bf16x3", "fp16"])
def test_whole_dnet_with_the_fp16_encoder(hip_lib, gpu, decoder_precision):
    from magnet_amd.dnet import DNET
    from magnet_amd.encoder import Encoder
    from magnet_amd.standin import make_dnet_args
    state, img, b, emu, plain = _dnet_case(gpu)
    hip = DNET(make_dnet_args(), Encoder(backend="hip", precision="fp16"), dnet=True, backend="hip", precision=decoder_precision)
    hip.load_state_dict(state)
    hip = hip.to(gpu).eval()
    with torch.no_grad():
        a = hip(img.to(gpu)).cpu()
    assert a.shape == b.shape == (2, 2, 64, 96) and bool(torch.isfinite(a).all())
    fails = []
    for ch, name in ((0, "mu"), (1, "variance")):
        top = float(b[:, ch].abs().max())
        err = float((a[:, ch] - b[:, ch]).abs().max()) / top
        e_emu = float((emu[:, ch] - plain[:, ch]).abs().max()) / float(plain[:, ch].abs().max())
        print(f"whole D-Net, fp16 encoder + {decoder_precision} decoder, {name}: max {top:.3g}, HIP - torch fp32 {err:.3g}, emulated taps through the "
              f"fp64 decoder {e_emu:.3g} of it (bar 2 x emulated)")
        if not err <= 2.0 * e_emu:
            fails.append((name, err, e_emu))
    assert not fails, f"over twice the emulated error (channel, HIP, emulated): {fails}"
