"""The D-Net's EfficientNet-B5 encoder without a GPU: the module's keys, parameter count and feature list, TF "SAME" padding, the
checkpoint round trip through DNET, and the host-side refusals of the new entry points and of MAGNET_ACT_SILU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def encoder():
    from magnet_amd.encoder import Encoder
    torch.manual_seed(0)
    return Encoder().eval()


def test_state_dict_keys_and_parameter_count(encoder):
    from magnet_amd import encoder as E
    sd = encoder.state_dict()
    assert all(k.startswith("original_model.") for k in sd)
    assert sum(p.numel() for p in encoder.parameters()) == 28_340_784 == E.PARAMETERS
    spot = {"conv_stem.weight": (48, 3, 3, 3), "bn1.running_mean": (48,), "bn1.num_batches_tracked": (),
            "blocks.0.0.conv_dw.weight": (48, 1, 3, 3), "blocks.0.0.se.conv_reduce.weight": (12, 48, 1, 1),
            "blocks.0.0.se.conv_reduce.bias": (12,), "blocks.0.0.conv_pw.weight": (24, 48, 1, 1), "blocks.0.1.se.conv_reduce.weight": (6, 24, 1, 1),
            "blocks.1.0.conv_pw.weight": (144, 24, 1, 1), "blocks.1.0.se.conv_reduce.weight": (6, 144, 1, 1),
            "blocks.1.1.se.conv_expand.weight": (240, 10, 1, 1), "blocks.2.0.conv_dw.weight": (240, 1, 5, 5),
            "blocks.3.6.bn3.weight": (128,), "blocks.4.0.se.conv_reduce.weight": (32, 768, 1, 1),
            "blocks.5.0.conv_dw.weight": (1056, 1, 5, 5), "blocks.5.8.conv_pwl.weight": (304, 1824, 1, 1),
            "blocks.6.0.se.conv_reduce.weight": (76, 1824, 1, 1), "blocks.6.2.se.conv_reduce.bias": (128,),
            "blocks.6.2.conv_pwl.weight": (512, 3072, 1, 1), "conv_head.weight": (2048, 512, 1, 1), "bn2.running_var": (2048,)}
    for k, shape in spot.items():
        assert tuple(sd["original_model." + k].shape) == shape, k
    assert not any("classifier" in k or "global_pool" in k for k in sd)
    assert [len(s) for s in encoder.original_model.blocks] == [3, 5, 5, 7, 7, 9, 3]
    assert all(m.eps == 1e-3 for m in encoder.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert all(m.bias is None for n, m in encoder.named_modules() if isinstance(m, torch.nn.Conv2d) and ".se." not in n)


def test_cpu_forward_returns_the_reference_feature_list(encoder):
    img = torch.rand(2, 3, 72, 104, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        f = encoder(img)
    assert len(f) == 16 and f[0] is img
    assert [t.shape[1] for t in f[1:14]] == [48, 48, 48, 24, 40, 64, 128, 176, 304, 512, 2048, 2048, 2048]
    sizes = {1: (36, 52), 4: (36, 52), 5: (18, 26), 6: (9, 13), 7: (5, 7), 8: (5, 7), 9: (3, 4), 10: (3, 4), 11: (3, 4), 15: (3, 4)}
    for i, hw in sizes.items():
        assert tuple(f[i].shape[2:]) == hw, i
    m = encoder.original_model
    with torch.no_grad():
        assert torch.equal(f[11], m.conv_head(f[10]))                                # raw: before bn2 and act2
        assert torch.equal(f[13], m.act2(m.bn2(f[11]))) and not torch.equal(f[11], f[13])
        assert torch.equal(f[15], f[13])                                             # global_pool, classifier: identities
        assert torch.equal(m(img), f[15])


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("L", [8, 9])
def test_tf_same_padding_is_asymmetric_on_even_sizes(k, L):
    from magnet_amd.encoder import Conv2dSame, same_pad
    g = torch.Generator().manual_seed(k * 10 + L)
    conv = Conv2dSame(4, 4, k, stride=2, groups=4)
    x = torch.randn(1, 4, L, L + 2, generator=g)
    pads = []
    for size in (L, L + 2):
        out = -(-size // 2)
        total = max((out - 1) * 2 + k - size, 0)
        pads.append((total // 2, total - total // 2))
        assert same_pad(size, k, 2) == pads[-1]
    assert pads[0] == {(3, 8): (0, 1), (5, 8): (1, 2), (3, 9): (1, 1), (5, 9): (2, 2)}[(k, L)]
    with torch.no_grad():
        got = conv(x)
        want = F.conv2d(F.pad(x, (pads[1][0], pads[1][1], pads[0][0], pads[0][1])), conv.weight, None, 2, 0, 1, 4)
        sym = F.conv2d(x, conv.weight, None, 2, k // 2, 1, 4)                         # the planted defect: symmetric padding
    assert got.shape == want.shape == (1, 4, -(-L // 2), -(-(L + 2) // 2)) and torch.equal(got, want)
    if L % 2 == 0:
        assert sym.shape == got.shape and not torch.allclose(sym, got)              # the defect is seen on an even size
    else:
        assert torch.equal(sym, got)


def test_dnet_builds_and_its_checkpoint_round_trips(tmp_path):
    from magnet_amd import magnet
    from magnet_amd.dnet import DNET, DNetMFMA
    from magnet_amd.encoder import Encoder
    from magnet_amd.standin import make_dnet_args
    torch.manual_seed(1)
    d = DNET(make_dnet_args(), Encoder()).eval()
    keys = list(d.state_dict())
    assert any(k.startswith("d_net.encoder.original_model.blocks.6.2.") for k in keys) and any(k.startswith("d_net.decoder.") for k in keys)
    for prefix in ("", "module."):
        path = str(tmp_path / f"dnet{len(prefix)}.pt")
        torch.save({"model": {prefix + k: v for k, v in d.state_dict().items()}}, path)
        other = DNET(make_dnet_args(), Encoder()).eval()
        magnet.load_checkpoint(path, other)
        assert all(torch.equal(v, other.state_dict()[k]) for k, v in d.state_dict().items())
    with torch.no_grad():
        feats = d.d_net.encoder(torch.rand(1, 3, 64, 96))
    runner = DNetMFMA(d.d_net.decoder)
    with pytest.raises(Exception, match="GPU"):                                       # the shapes pass; only the device is refused
        runner._features(feats)
    assert [tuple(feats[i].shape[1:]) for i in (5, 6, 8, 11)] == [(40, 16, 24), (64, 8, 12), (176, 4, 6), (2048, 2, 3)]


def test_seeded_encoder_is_deterministic_and_calibrated():
    from magnet_amd.encoder import Encoder, load_seeded_encoder, seeded_encoder_state
    a, b = seeded_encoder_state(3), seeded_encoder_state(3)
    assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(Encoder().state_dict())
    assert not torch.equal(a["original_model.conv_stem.weight"], seeded_encoder_state(4)["original_model.conv_stem.weight"])
    enc = Encoder()
    enc.load_state_dict(a)
    assert all(torch.equal(v, a[k]) for k, v in load_seeded_encoder(Encoder(), 3).state_dict().items())
    enc.eval()
    with torch.no_grad():
        f = enc(torch.rand(2, 3, 72, 104, generator=torch.Generator().manual_seed(2)))
    for i in (4, 5, 6, 8, 11):                                                        # of order 1: no blow-up, no collapse
        assert 0.1 < float(f[i].std()) < 30.0, (i, float(f[i].std()))


def test_standin_make_dnet_takes_the_b5_encoder():
    from magnet_amd.encoder import Encoder
    from magnet_amd.standin import StandinEncoder, make_dnet
    assert isinstance(make_dnet().d_net.encoder, StandinEncoder)                      # the default stays what it is
    d = make_dnet(encoder="b5")
    assert isinstance(d.d_net.encoder, Encoder) and not d.training
    with pytest.raises(Exception, match="encoder"):
        make_dnet(encoder="b7")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_act_silu_constant_matches_the_header():
    from magnet_amd import lib
    hdr = open(os.path.join(REPO, "include", "magnet_hip.h")).read()
    assert int(re.search(r"MAGNET_ACT_SILU\s*=\s*(\d+)", hdr).group(1)) == lib.ACT_SILU == 2


def _conv_ex(lib, **kw):
    x = lib.MagnetConvExArgs()
    c = x.base
    c.in_hi = c.in_lo = c.w_hi = c.w_lo = c.bias = c.out_hi = c.out_lo = c.out_f32 = 16
    c.rows, c.cin, c.cout_pad, c.taps, c.wp, c.out_mode = 128, 64, 128, 1, 10, 1
    x.act = lib.ACT_SILU
    for k, v in kw.items():
        setattr(c if hasattr(c, k) else x, k, v)
    return x


def test_act_silu_refusals(hip_lib):
    from magnet_amd import lib
    L = hip_lib
    err = lambda: L.magnet_last_error().decode()
    x = _conv_ex(lib, relu=1)
    assert L.magnet_conv_mfma_ex(ctypes.byref(x), None) == lib.E_DIM and "SiLU excludes relu" in err()
    x = _conv_ex(lib, tail_w_hi=16)
    assert L.magnet_conv_mfma_ex(ctypes.byref(x), None) == lib.E_DIM and "SiLU excludes relu and the fused tail" in err()
    x = _conv_ex(lib); x.act = 7
    assert L.magnet_conv_mfma_ex(ctypes.byref(x), None) == lib.E_DIM and err() == "magnet_conv_mfma_ex: act=7 unknown"
    work = (ctypes.c_float * 4)()
    for name, call in (("magnet_conv_mfma_f16", lambda a: L.magnet_conv_mfma_f16(a, None)),
                       ("magnet_conv_mfma_f16p", lambda a: L.magnet_conv_mfma_f16p(a, None)),
                       ("magnet_conv_mfma_f16d", lambda a: L.magnet_conv_mfma_f16d(a, None)),
                       ("magnet_conv_mfma_splitk", lambda a: L.magnet_conv_mfma_splitk(a, 2, ctypes.addressof(work), 1 << 40, None)),
                       ("magnet_conv_mfma_f16d_splitk", lambda a: L.magnet_conv_mfma_f16d_splitk(a, 2, ctypes.addressof(work), 1 << 40, None))):
        x = _conv_ex(lib, cin=256)
        if "f16" in name:
            x.base.in_lo = x.base.w_lo = None
        if name == "magnet_conv_mfma_f16":
            x.base.taps = 9
        work[0] = 123.0
        assert call(ctypes.byref(x)) == lib.E_DIM, (name, err())
        assert name in err() and "act=2" in err(), err()
        assert work[0] == 123.0
    for query in (L.magnet_conv_mfma_splitk_workspace, L.magnet_conv_mfma_f16d_splitk_workspace):
        x = _conv_ex(lib, cin=256); x.act = lib.ACT_BASE
        if query is L.magnet_conv_mfma_f16d_splitk_workspace:
            x.base.in_lo = x.base.w_lo = None
        assert query(ctypes.byref(x), 2) == 2 * 128 * 128 * 4                         # the form itself is served: only the activation is refused


def _dw(lib, **kw):
    a = lib.MagnetDwConvArgs()
    a.in_hi = a.in_lo = a.wgt = a.bias = a.out_hi = a.out_lo = a.part = 16
    a.N, a.h, a.w, a.c_pad, a.in_ld, a.out_ld, a.k, a.stride, a.pad_top, a.pad_left = 2, 9, 13, 64, 64, 64, 3, 2, 1, 1
    a.n_part = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_dwconv_refusals(hip_lib):
    from magnet_amd import lib
    L = hip_lib
    err = lambda: L.magnet_last_error().decode()
    assert lib.dwconv_parts(5, 7) == 1 and lib.dwconv_parts(8, 16) == 1 and lib.dwconv_parts(9, 17) == 4 and lib.dwconv_parts(120, 160) == 150
    assert lib.dwconv_parts(0, 5) == 0
    assert L.magnet_dwconv_cl(None, None) == lib.E_NULL and "args is NULL" in err()
    cases = [(dict(part=None), lib.E_NULL, "NULL pointer"), (dict(in_lo=None), lib.E_NULL, "NULL pointer"),
             (dict(k=4), lib.E_DIM, "k=4"), (dict(k=7), lib.E_DIM, "k=7"), (dict(stride=3), lib.E_DIM, "stride=3"), (dict(stride=0), lib.E_DIM, "stride=0"),
             (dict(c_pad=48, in_ld=48, out_ld=48), lib.E_DIM, "c_pad=48"), (dict(N=0), lib.E_DIM, "bad dims"), (dict(h=0), lib.E_DIM, "bad dims"),
             (dict(in_ld=32), lib.E_DIM, "in_ld=32"), (dict(out_ld=68), lib.E_DIM, "out_ld=68"), (dict(pad_top=3), lib.E_DIM, "pad_top=3"),
             (dict(pad_left=-1), lib.E_DIM, "pad_left=-1"), (dict(n_part=2), lib.E_DIM, "n_part=2"),
             (dict(h=40000, w=40000), lib.E_DIM, "2^31"),
             (dict(in_hi=24), lib.E_ALIGN, "16-byte"), (dict(out_lo=8), lib.E_ALIGN, "16-byte"), (dict(wgt=4), lib.E_ALIGN, "16-byte"),
             (dict(part=18), lib.E_ALIGN, "4-byte")]
    for kw, code, what in cases:
        assert L.magnet_dwconv_cl(ctypes.byref(_dw(lib, **kw)), None) == code, (kw, err())
        assert "magnet_dwconv_cl" in err() and what in err(), (kw, err())
    with pytest.raises(lib.MagnetError, match="bf16 GPU tensor"):
        z = torch.zeros(8, 64)
        lib.dwconv_cl(z, z, 64, 1, 2, 2, 64, z, z, 3, 1, 1, 1, z, z, 64, z)


def test_stem_gate_and_scale_refusals(hip_lib):
    from magnet_amd import lib
    L = hip_lib
    err = lambda: L.magnet_last_error().decode()
    assert L.magnet_enc_stem(16, 16, None, 16, 16, 1, 8, 8, None) == lib.E_NULL and "magnet_enc_stem" in err()
    assert L.magnet_enc_stem(16, 16, 16, 16, 16, 0, 8, 8, None) == lib.E_DIM and "N=0" in err()
    assert L.magnet_enc_stem(16, 16, 16, 16, 16, 1, 1, 8, None) == lib.E_DIM and "H=1" in err()
    assert L.magnet_enc_stem(16, 16, 16, 16, 24, 1, 8, 8, None) == lib.E_ALIGN and "16-byte" in err()
    gate = lambda **kw: L.magnet_se_gate(*[{**dict(part=16, n_part=3, hw=35, w1=16, b1=16, w2=16, b2=16, C=48, R=12, c_pad=64, gate=16, N=2), **kw}[k]
                                           for k in ("part", "n_part", "hw", "w1", "b1", "w2", "b2", "C", "R", "c_pad", "gate", "N")], None)
    assert gate(gate=None) == lib.E_NULL and "magnet_se_gate: NULL" in err()
    for kw, what in ((dict(n_part=0), "n_part=0"), (dict(hw=0), "hw=0"), (dict(C=65), "C=65"), (dict(C=8224, c_pad=8224), "C=8224"), (dict(R=0), "R=0"),
                     (dict(R=1025), "R=1025"), (dict(c_pad=48), "c_pad=48"), (dict(N=0), "N=0")):
        assert gate(**kw) == lib.E_DIM and what in err(), (kw, err())
    assert gate(part=20) == lib.E_ALIGN and "16-byte" in err()
    assert gate(gate=18) == lib.E_ALIGN and "4-byte" in err()
    scale = lambda **kw: L.magnet_se_scale(*[{**dict(ih=16, il=16, in_ld=64, gate=16, N=2, h=5, w=7, c_pad=64, oh=16, ol=16, out_ld=64), **kw}[k]
                                             for k in ("ih", "il", "in_ld", "gate", "N", "h", "w", "c_pad", "oh", "ol", "out_ld")], None)
    assert scale(ol=None) == lib.E_NULL and "magnet_se_scale: NULL" in err()
    for kw, what in ((dict(c_pad=40, in_ld=40, out_ld=40), "c_pad=40"), (dict(in_ld=32), "in_ld=32"), (dict(out_ld=68), "out_ld=68"), (dict(w=0), "w=0")):
        assert scale(**kw) == lib.E_DIM and what in err(), (kw, err())
    assert scale(gate=20) == lib.E_ALIGN and "16-byte" in err()
    assert scale(ih=8) == lib.E_ALIGN


def test_runner_refuses_cpu_tensors_and_train_mode(hip_lib):
    from magnet_amd import lib
    from magnet_amd.encoder import Encoder, EncoderMFMA, cout_pad_of
    enc = Encoder(backend="hip")
    img = torch.rand(1, 3, 64, 96)
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        enc.eval()(img)
    with torch.no_grad():
        assert len(enc.train()(img)) == 16                                            # a .train() forward runs the torch modules
    with pytest.raises(lib.MagnetError, match="backend"):
        Encoder(backend="cuda")
    assert [cout_pad_of(c) for c in (24, 40, 64, 128, 144, 176, 240, 304, 384, 512, 768, 1056, 1824, 2048, 3072)] == \
        [32, 64, 64, 128, 144, 256, 256, 384, 384, 512, 768, 1152, 1920, 2048, 3072]
    assert isinstance(enc._runner, EncoderMFMA)
