"""The encoder's fp16 single-plane mode without a GPU: the four new entry points are exported, typed and refuse bad arguments on the
host under their own names; the older fp16 routes keep refusing SiLU; the precision keyword of Encoder, EncoderMFMA and make_dnet; the
eval drivers' flag; the out-of-range folded weight; and the ABI version, which additions do not move."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("magnet_conv_mfma_f16e", "magnet_enc_stem_f16", "magnet_dwconv_cl_f16", "magnet_se_scale_f16")


def test_new_symbols_are_exported_and_typed(hip_lib):
    from magnet_amd import lib
    hdr = open(os.path.join(REPO, "include", "magnet_hip.h")).read()
    for s in NEW:
        assert s in lib.API_SYMBOLS and hasattr(hip_lib, s), s
        fn = getattr(hip_lib, s)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and fn.argtypes[-1] is ctypes.c_void_p, s
        assert re.search(r"^MAGNET_API int %s\(" % s, hdr, flags=re.M), s
    assert len(hip_lib.magnet_enc_stem_f16.argtypes) == 8 and len(hip_lib.magnet_se_scale_f16.argtypes) == 10
    assert lib._CONV_ROUTES["enc"][0] == "magnet_conv_mfma_f16e"


def test_version_literal_is_still_500(hip_lib):
    hdr = open(os.path.join(REPO, "include", "magnet_hip.h")).read()
    assert int(re.search(r"#define\s+MAGNET_HIP_VERSION\s+(\d+)", hdr).group(1)) == 500 == hip_lib.magnet_version()
    assert all(s in hdr.split("typedef")[0] for s in NEW), "the header's version comment records the additions"


def _conv(lib, **kw):
    """A valid magnet_conv_mfma_f16e call but for the pointers (16 = aligned, never dereferenced: every case below is refused)."""
    x = lib.MagnetConvExArgs()
    c = x.base
    c.in_hi = c.w_hi = c.bias = c.out_hi = c.out_f32 = 16
    c.rows, c.cin, c.cout_pad, c.taps, c.wp, c.out_mode = 128, 64, 128, 1, 10, 3
    x.act = lib.ACT_SILU
    for k, v in kw.items():
        setattr(c if hasattr(c, k) else x, k, v)
    return x


def test_conv_f16e_host_refusals(hip_lib):
    from magnet_amd import lib
    L = hip_lib
    err = lambda: L.magnet_last_error().decode()
    assert L.magnet_conv_mfma_f16e(None, None) == lib.E_NULL and err().startswith("magnet_conv_mfma_f16e")
    cases = [(dict(in_lo=16), "in_lo"), (dict(w_lo=16), "in_lo"), (dict(add_lo=16), "add_lo"), (dict(add_hi=16, add_lo=16), "add_lo"),
             (dict(taps=9), "taps=9"), (dict(taps=4), "taps=4"), (dict(taps=1, dil=2), "dil=2"),
             (dict(cout_pad=144), "cout_pad=144"), (dict(cout_pad=16), "cout_pad=16"), (dict(cout_pad=192), "cout_pad=192"),
             (dict(relu=1), "relu=1"), (dict(act=lib.ACT_BASE, relu=1), "relu=1"), (dict(act=lib.ACT_LEAKY_RELU, act_slope=0.1), "act=1"),
             (dict(act=7), "act=7"), (dict(tail_w_hi=16), "fused tail"), (dict(addend=16), "addend"), (dict(gu_out=16), "Gaussian update"),
             (dict(up_out=16), "upsampling"), (dict(tiling=lib.TILING_BM64), "tiling=%d" % lib.TILING_BM64),
             (dict(tiling=lib.TILING_BM256), "tiling=%d" % lib.TILING_BM256),
             (dict(out_mode=0), "out_mode=0"), (dict(out_mode=2), "out_mode=2")]
    for kw, what in cases:
        assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, **kw)), None) == lib.E_DIM, (kw, err())
        assert err().startswith("magnet_conv_mfma_f16e:") and what in err(), (kw, err())
    # the common fields: codes as every convolution entry point gives them
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, in_hi=None)), None) == lib.E_NULL
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, out_hi=None)), None) == lib.E_NULL
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, out_mode=1, out_f32=None)), None) == lib.E_NULL
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, in_hi=24)), None) == lib.E_ALIGN
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, add_hi=8)), None) == lib.E_ALIGN
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, cin=48)), None) == lib.E_DIM
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, rows=0)), None) == lib.E_DIM
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, out_ld=64)), None) == lib.E_DIM and "out_ld=64" in err()
    assert L.magnet_conv_mfma_f16e(ctypes.byref(_conv(lib, add_hi=16, add_ld=64)), None) == lib.E_ALIGN
    with pytest.raises(lib.MagnetError, match="fp16 GPU tensor"):
        z = torch.zeros(8, 64, dtype=torch.float16)
        lib.conv_mfma(z, None, 64, 64, z[None], None, torch.zeros(64), 1, 4, False, 8, out_hi=z, f16="enc")
    with pytest.raises(lib.MagnetError, match="f16='enc'"):
        lib.conv_mfma(None, None, 64, 64, None, None, None, 1, 4, True, 8, f16="enc")


def test_older_fp16_routes_still_refuse_silu(hip_lib):
    """The contracts magnet_conv_mfma_f16e was added to leave alone."""
    from magnet_amd import lib
    L = hip_lib
    for fn, name in ((L.magnet_conv_mfma_f16p, "magnet_conv_mfma_f16p"), (L.magnet_conv_mfma_f16d, "magnet_conv_mfma_f16d")):
        assert fn(ctypes.byref(_conv(lib)), None) == lib.E_DIM
        e = L.magnet_last_error().decode()
        assert name + ":" in e and "act=2" in e, e
    # and the wide route still has no residual input
    assert L.magnet_conv_mfma_f16d(ctypes.byref(_conv(lib, act=lib.ACT_BASE, add_hi=16)), None) == lib.E_DIM


def _dw(lib, **kw):
    a = lib.MagnetDwConvArgs()
    a.in_hi = a.wgt = a.bias = a.out_hi = a.part = 16
    a.N, a.h, a.w, a.c_pad, a.in_ld, a.out_ld, a.k, a.stride, a.pad_top, a.pad_left = 2, 9, 13, 64, 64, 64, 3, 2, 1, 1
    a.n_part = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_dwconv_f16_host_refusals(hip_lib):
    from magnet_amd import lib
    L = hip_lib
    err = lambda: L.magnet_last_error().decode()
    assert L.magnet_dwconv_cl_f16(None, None) == lib.E_NULL and err() == "magnet_dwconv_cl_f16: args is NULL"
    cases = [(dict(part=None), lib.E_NULL, "NULL pointer"), (dict(in_hi=None), lib.E_NULL, "NULL pointer"), (dict(out_hi=None), lib.E_NULL, "NULL pointer"),
             (dict(in_lo=16), lib.E_DIM, "in_lo and out_lo must be NULL"), (dict(out_lo=16), lib.E_DIM, "in_lo and out_lo must be NULL"),
             (dict(k=4), lib.E_DIM, "k=4"), (dict(stride=3), lib.E_DIM, "stride=3"), (dict(c_pad=48, in_ld=48, out_ld=48), lib.E_DIM, "c_pad=48"),
             (dict(N=0), lib.E_DIM, "bad dims"), (dict(in_ld=32), lib.E_DIM, "in_ld=32"), (dict(out_ld=68), lib.E_DIM, "out_ld=68"),
             (dict(pad_top=3), lib.E_DIM, "pad_top=3"), (dict(n_part=2), lib.E_DIM, "n_part=2"), (dict(h=40000, w=40000), lib.E_DIM, "2^31"),
             (dict(in_hi=24), lib.E_ALIGN, "16-byte"), (dict(out_hi=8), lib.E_ALIGN, "16-byte"), (dict(wgt=4), lib.E_ALIGN, "16-byte"),
             (dict(part=18), lib.E_ALIGN, "4-byte")]
    for kw, code, what in cases:
        assert L.magnet_dwconv_cl_f16(ctypes.byref(_dw(lib, **kw)), None) == code, (kw, err())
        assert err().startswith("magnet_dwconv_cl_f16:") and what in err(), (kw, err())
    with pytest.raises(lib.MagnetError, match="fp16 GPU tensor"):
        z = torch.zeros(8, 64)
        lib.dwconv_cl_f16(z, 64, 1, 2, 2, 64, z, z, 3, 1, 1, 1, z, 64, z)


def test_stem_and_scale_f16_host_refusals(hip_lib):
    from magnet_amd import lib
    L = hip_lib
    err = lambda: L.magnet_last_error().decode()
    assert L.magnet_enc_stem_f16(16, 16, None, 16, 1, 8, 8, None) == lib.E_NULL and err() == "magnet_enc_stem_f16: NULL pointer"
    assert L.magnet_enc_stem_f16(16, 16, 16, None, 1, 8, 8, None) == lib.E_NULL
    assert L.magnet_enc_stem_f16(16, 16, 16, 16, 0, 8, 8, None) == lib.E_DIM and err().startswith("magnet_enc_stem_f16:") and "N=0" in err()
    assert L.magnet_enc_stem_f16(16, 16, 16, 16, 1, 1, 8, None) == lib.E_DIM and "H=1" in err()
    assert L.magnet_enc_stem_f16(16, 16, 16, 24, 1, 8, 8, None) == lib.E_ALIGN and err().startswith("magnet_enc_stem_f16:") and "16-byte" in err()
    scale = lambda **kw: L.magnet_se_scale_f16(*[{**dict(i=16, in_ld=64, gate=16, N=2, h=5, w=7, c_pad=64, o=16, out_ld=64), **kw}[k]
                                                 for k in ("i", "in_ld", "gate", "N", "h", "w", "c_pad", "o", "out_ld")], None)
    assert scale(o=None) == lib.E_NULL and err() == "magnet_se_scale_f16: NULL pointer"
    assert scale(i=None) == lib.E_NULL and scale(gate=None) == lib.E_NULL
    for kw, what in ((dict(c_pad=40, in_ld=40, out_ld=40), "c_pad=40"), (dict(in_ld=32), "in_ld=32"), (dict(out_ld=68), "out_ld=68"), (dict(w=0), "w=0")):
        assert scale(**kw) == lib.E_DIM and err().startswith("magnet_se_scale_f16:") and what in err(), (kw, err())
    assert scale(gate=20) == lib.E_ALIGN and "16-byte" in err()
    assert scale(i=8) == lib.E_ALIGN and err().startswith("magnet_se_scale_f16:")
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        lib.se_scale_f16(torch.zeros(8, 64), 64, torch.zeros(1, 64), 1, 2, 2, 64, torch.zeros(8, 64), 64)
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        lib.enc_stem_f16(torch.zeros(1, 3, 8, 8), torch.zeros(48, 27), torch.zeros(48), torch.zeros(1, dtype=torch.float16))


def test_precision_keyword_validation(hip_lib):
    from magnet_amd import encoder as E
    from magnet_amd import lib
    from magnet_amd.standin import make_dnet
    assert E.PRECISIONS == ("bf16x3", "fp16")
    assert E.Encoder().precision == "bf16x3" and E.Encoder(backend="hip")._runner.precision == "bf16x3"
    enc = E.Encoder(backend="hip", precision="fp16")
    assert enc.precision == "fp16" and isinstance(enc._runner, E.EncoderMFMA) and enc._runner.precision == "fp16"
    with torch.no_grad():
        assert len(enc.train()(torch.rand(1, 3, 64, 96))) == 16                       # a .train() forward still runs the torch modules
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        enc.eval()(torch.rand(1, 3, 64, 96))
    with pytest.raises(lib.MagnetError, match="backend='hip'"):
        E.Encoder(backend="torch", precision="fp16")
    for bad in ("fp32", "FP16", None, 16):
        with pytest.raises(lib.MagnetError, match="precision"):
            E.Encoder(backend="hip", precision=bad)
        with pytest.raises(lib.MagnetError, match="precision"):
            E.EncoderMFMA(enc.original_model, precision=bad)
    assert E.EncoderMFMA(enc.original_model).precision == "bf16x3"
    for kw in (dict(), dict(encoder="b5"), dict(encoder="standin", encoder_backend="torch"), dict(encoder="b5", encoder_backend="torch")):
        with pytest.raises(ValueError, match="encoder_precision"):
            make_dnet(encoder_precision="fp16", **kw)
    assert make_dnet(encoder_precision="bf16x3").d_net.encoder is not None            # the default value passes everywhere
    d = make_dnet(encoder="b5", encoder_backend="hip", encoder_precision="fp16")
    assert d.d_net.encoder._runner.precision == "fp16" and not d.training
    with pytest.raises(lib.MagnetError, match="precision"):
        make_dnet(encoder="b5", encoder_backend="hip", encoder_precision="fp8")


def test_fp16_pack_slices_and_out_of_range_weight():
    """The pack needs no GPU: one fp16 plane per layer, 144 outputs as 128 + 32 in a 160-wide buffer, and a folded weight beyond fp16's
    range is an error that names the layer."""
    from magnet_amd import encoder as E
    from magnet_amd import lib
    torch.manual_seed(0)
    enc = E.Encoder(backend="hip", precision="fp16").eval()
    P = enc._runner._pack(torch.device("cpu"))
    w, lo, bias, cout, slices = P["blocks.1.0.pw"]
    assert lo is None and w.dtype == torch.float16 and tuple(w.shape) == (1, 160, 32) and cout == 144 and tuple(bias.shape) == (160,)
    assert [(c0, tuple(ws.shape), tuple(bs.shape)) for c0, ws, bs in slices] == [(0, (1, 128, 32), (128,)), (128, (1, 32, 32), (32,))]
    assert torch.equal(torch.cat([s[1] for s in slices], 1), w) and bool((w[:, 144:] == 0).all()) and bool((w[:, :, 24:] == 0).all())
    widths = sorted({P[k][0].shape[1] for k in P if k.endswith((".pw", ".pwl")) or k == "conv_head"})
    assert widths == [32, 64, 128, 160, 256, 384, 512, 768, 1152, 1920, 2048, 3072]
    assert all(len(P[k][4]) == 1 and P[k][4][0][1].shape == P[k][0].shape for k in P if k.endswith(".pwl"))
    fold, _ = E.fold_bn(enc.original_model.blocks[2][1].conv_pwl, enc.original_model.blocks[2][1].bn3)
    assert torch.equal(P["blocks.2.1.pwl"][0][0, :64, :384], fold.float().reshape(64, 384).to(torch.float16))   # rounded once, after the fp64 fold
    assert P["blocks.2.1.dw"][0].dtype == torch.float32 and P["blocks.2.1.se"][0].dtype == torch.float32       # depthwise and squeeze-excite stay fp32
    # the two precisions' packs live side by side in the runner's cache (keyed by precision)
    r = enc._runner
    p16 = r.packed(torch.device("cpu"))
    r.precision = "bf16x3"
    p32 = r.packed(torch.device("cpu"))
    r.precision = "fp16"
    assert r.packed(torch.device("cpu")) is p16 and p32 is not p16 and len(p32["blocks.1.0.pw"]) == 4
    with torch.no_grad():
        enc.original_model.blocks[3][2].conv_pwl.weight[5, 7] = 3.0e5
    with pytest.raises(lib.MagnetError, match=r"blocks\.3\.2\.pwl.*outside fp16's range"):
        r._pack(torch.device("cpu"))
    r.precision = "bf16x3"
    assert "blocks.3.2.pwl" in r._pack(torch.device("cpu"))                           # the default mode holds the same module


@pytest.mark.parametrize("driver", ["eval_dnet.py", "eval_synthetic.py"])
def test_eval_drivers_refuse_the_flag_without_the_hip_b5_encoder(driver):
    for extra in ([], ["--encoder", "b5"]):                                          # the stand-in, and b5 on its default torch backend
        p = subprocess.run([sys.executable, os.path.join(REPO, driver), "--encoder_precision", "fp16"] + extra, capture_output=True, text=True, cwd=REPO)
        assert p.returncode == 2 and "--encoder_precision fp16 is a mode of --encoder b5 --encoder_backend hip" in p.stderr, p.stderr[-400:]
    p = subprocess.run([sys.executable, os.path.join(REPO, driver), "--encoder_precision", "fp8"], capture_output=True, text=True, cwd=REPO)
    assert p.returncode == 2 and "invalid choice" in p.stderr
