"""The host side of the D-Net decoder's fp16 single-plane mode: the precision arguments of DNetMFMA, DNET and MAGNET, the fp16 weight
pack (layout, bits, one pack per precision, the 65504 check), the new prototypes, the workspace query of magnet_conv_mfma_f16d_splitk
and the argument errors of the two new entry points as codes.  No GPU needed: every refusal comes before a launch."""
import ctypes

import pytest
import torch

from magnet_amd import lib
from magnet_amd.dnet import DNET, DNetMFMA, _UP
from magnet_amd.magnet import MAGNET
from magnet_amd.planes import fold_bn, pack_taps_f16, round_up
from magnet_amd.standin import StandinEncoder, StubFNet, make_args, make_dnet, make_dnet_args


def test_runner_precision_argument():
    dec = make_dnet().d_net.decoder
    assert DNetMFMA(dec).precision == "bf16x3"                               # the default does not move
    assert DNetMFMA(dec, precision="bf16x3").precision == "bf16x3"
    r = DNetMFMA(dec, precision="fp16")
    assert r.precision == "fp16" and r.launch_log == []
    for sk in ("auto", {"up1.0": 2, "up2.0": 2}):                            # composes with split_k
        r = DNetMFMA(dec, split_k=sk, precision="fp16")
        assert r.precision == "fp16" and r.split_k == sk
    for bad in ("fp32", "f16", "FP16", None, 16, True, ("fp16",)):
        with pytest.raises(lib.MagnetError, match="must be 'bf16x3' or 'fp16'"):
            DNetMFMA(dec, precision=bad)


def test_dnet_precision_argument():
    for dn in (False, True):
        assert DNET(make_dnet_args(), StandinEncoder(), dnet=dn).precision == "bf16x3"
        assert DNET(make_dnet_args(), StandinEncoder(), dnet=dn, backend="hip")._runner.precision == "bf16x3"
        d = DNET(make_dnet_args(), StandinEncoder(), dnet=dn, backend="hip", precision="fp16")
        assert d.precision == "fp16" and d._runner.precision == "fp16"
        d = DNET(make_dnet_args(), StandinEncoder(), dnet=dn, backend="hip", split_k="auto", precision="fp16")
        assert d._runner.precision == "fp16" and d._runner.split_k == "auto"
    with pytest.raises(lib.MagnetError, match="must be 'bf16x3' or 'fp16'"):
        DNET(make_dnet_args(), StandinEncoder(), backend="hip", precision="half")
    with pytest.raises(lib.MagnetError, match="backend='hip'"):
        DNET(make_dnet_args(), StandinEncoder(), precision="fp16")            # the torch backend has no such mode
    assert DNET(make_dnet_args(), StandinEncoder(), precision="bf16x3")._runner is None


def test_magnet_dnet_precision_argument():
    d = make_dnet()
    mk = lambda **kw: MAGNET(make_args(), d_net=d, f_net=StubFNet(), **kw)
    assert mk().dnet_precision == "bf16x3"
    m = mk(dnet_backend="hip")
    assert m.dnet_precision == "bf16x3" and m._dnet.precision == "bf16x3"
    m = mk(dnet_backend="hip", dnet_precision="fp16")
    assert m.dnet_precision == "fp16" and m._dnet.precision == "fp16"
    assert m.conv_precision == "bf16x3" and m.fnet_precision == "bf16x3"       # independent of the other two precision modes
    m = mk(dnet_backend="hip", dnet_precision="fp16", dnet_split_k="auto", conv_precision="fp16", fnet_precision="fp16")
    assert (m._dnet.precision, m._dnet.split_k, m.conv_precision, m.fnet_precision) == ("fp16", "auto", "fp16", "fp16")
    m = mk(dnet_backend="hip", conv_precision="fp16")
    assert m._dnet.precision == "bf16x3"
    with pytest.raises(lib.MagnetError, match="dnet_precision must be 'bf16x3' or 'fp16'"):
        mk(dnet_backend="hip", dnet_precision="bf16")
    with pytest.raises(lib.MagnetError, match="dnet_backend='hip'"):
        mk(dnet_precision="fp16")


def _folds(dec):
    out = [("conv2", dec.conv2.weight.detach().double(), dec.conv2.bias.detach().double(), 2048)]
    cin = 2048
    for name, _, skip_c, cout in _UP:
        net = getattr(dec, name)._net
        out.append((name + ".0",) + fold_bn(net[0], net[1]) + (round_up(cin + skip_c, 32),))
        out.append((name + ".1",) + fold_bn(net[3], net[4]) + (cout,))
        cin = cout
    return out


def test_fp16_weight_pack_is_pack_taps_f16_of_the_fp64_fold():
    dec = make_dnet().d_net.decoder                                           # the seeded decoder
    r = DNetMFMA(dec, precision="fp16")
    P = r.packed(torch.device("cpu"))
    assert set(P) == {"conv2", "up1.0", "up1.1", "up2.0", "up2.1", "up3.0", "up3.1"}
    for name, w, b, cin_pad in _folds(dec):
        hi, lo, bias, taps, cin = P[name]
        exp = pack_taps_f16(w.float(), cin_pad)
        assert lo is None and hi.dtype == torch.float16 and hi.is_contiguous()
        assert tuple(hi.shape) == (9 if name != "conv2" else 1, w.shape[0], cin_pad) and (taps, cin) == (hi.shape[0], cin_pad)
        assert torch.equal(hi.view(torch.int16), exp.view(torch.int16)), name
        assert bias.dtype == torch.float32 and torch.equal(bias, b.float())   # biases stay fp32
        if cin_pad != w.shape[1]:
            assert not hi[:, :, w.shape[1]:].any()                            # the padding channels are zero
        # each weight is within half an fp16 ulp of the fold (relative 2^-11 in the normal range)
        wt = w.permute(2, 3, 0, 1).reshape(hi.shape[0], w.shape[0], w.shape[1])
        err = (hi[:, :, :w.shape[1]].double() - wt).abs()
        assert bool((err <= wt.abs() * 2.0 ** -11 + 2.0 ** -25).all())


def test_pack_cache_keeps_one_pack_per_precision():
    dec = make_dnet().d_net.decoder
    r = DNetMFMA(dec, precision="fp16")
    cpu = torch.device("cpu")
    p16 = r.packed(cpu)
    assert r.packed(cpu) is p16                                               # cached
    r.precision = "bf16x3"
    p3 = r.packed(cpu)
    assert p3 is not p16 and p3["conv2"][0].dtype == torch.bfloat16 and p3["conv2"][1] is not None
    r.precision = "fp16"
    assert r.packed(cpu) is p16 and r._cache.get(cpu, lambda: None, "bf16x3") is p3    # both packs live side by side
    with torch.no_grad():
        dec.conv2.bias.add_(1.0)                                              # an in-place update invalidates both
    assert r.packed(cpu) is not p16
    # the default mode's pack is what it was: the split-bf16 pair of pack_taps
    from magnet_amd.planes import pack_taps
    q = DNetMFMA(dec).packed(cpu)
    hi, lo = pack_taps(dec.conv2.weight.detach().double(), 2048)
    assert torch.equal(q["conv2"][0].view(torch.int16), hi.view(torch.int16)) and torch.equal(q["conv2"][1].view(torch.int16), lo.view(torch.int16))


def test_a_folded_weight_beyond_fp16_raises_at_pack_time():
    dec = make_dnet().d_net.decoder
    with torch.no_grad():
        dec.up2._net[3].weight[5, 7, 1, 1] = 7.0e4                            # folded by gamma / sqrt(var + eps) in [0.42, 1.98]: push it out
        s = dec.up2._net[4].weight[5] / torch.sqrt(dec.up2._net[4].running_var[5] + dec.up2._net[4].eps)
        dec.up2._net[3].weight[5, 7, 1, 1] = 7.0e4 / float(s)
    with pytest.raises(lib.MagnetError, match=r"up2\.1.*65504"):
        DNetMFMA(dec, precision="fp16").packed(torch.device("cpu"))
    DNetMFMA(dec).packed(torch.device("cpu"))                                 # the default mode has no such limit
    with torch.no_grad():
        dec.up2._net[3].weight[5, 7, 1, 1] = 6.0e4 / float(s)                 # inside the range: packs, not clamped
    P = DNetMFMA(dec, precision="fp16").packed(torch.device("cpu"))
    assert abs(float(P["up2.1"][0][4, 5, 7]) - 6.0e4) <= 6.0e4 * 2.0 ** -11 + 32


def test_new_prototypes_are_declared(hip_lib):
    for name, proto in (("magnet_conv_mfma_f16d", (lib._C, [lib._S(lib.MagnetConvExArgs), lib._P])),
                        ("magnet_conv_mfma_f16d_splitk_workspace", (lib._L, [lib._S(lib.MagnetConvExArgs), lib._I])),
                        ("magnet_conv_mfma_f16d_splitk", (lib._C, [lib._S(lib.MagnetConvExArgs), lib._I, lib._P, lib._L, lib._P]))):
        assert lib._PROTOS[name] == proto and name in lib.API_SYMBOLS
        f = getattr(hip_lib, name)
        assert f.restype is proto[0] and list(f.argtypes) == proto[1]


def _valid():
    x = lib.MagnetConvExArgs()
    b = x.base
    b.in_hi = b.w_hi = b.bias = b.out_hi = b.out_f32 = 16                       # non-NULL, 16-byte aligned; nothing is dereferenced
    b.rows, b.cin, b.cout_pad, b.taps, b.wp, b.out_mode, b.in_ld = 330, 160, 256, 9, 15, 3, 160
    return x


def test_workspace_query_of_the_fp16_split_k_form(hip_lib):
    L = hip_lib
    ws = L.magnet_conv_mfma_f16d_splitk_workspace
    for S in (2,):
        assert ws(ctypes.byref(_valid()), S) == S * 330 * 256 * 4
    x = _valid(); x.base.cin = 512
    for S in (2, 3, 8):
        assert ws(ctypes.byref(x), S) == S * 330 * 256 * 4
    assert lib.conv_mfma_splitk_workspace(330, 160, 256, 9, 2, f16="wide") == 2 * 330 * 256 * 4
    assert lib.conv_mfma_splitk_workspace(330, 160, 256, 1, 2, f16="wide") == lib.conv_mfma_splitk_workspace(330, 160, 256, 1, 2)
    with pytest.raises(lib.MagnetError) as e:
        lib.conv_mfma_splitk_workspace(330, 160, 256, 9, 3, f16="wide")        # 5 chunks over 3 splits
    assert e.value.code == lib.E_DIM
    with pytest.raises(lib.MagnetError, match="f16 must be False or 'wide'"):
        lib.conv_mfma_splitk_workspace(330, 160, 256, 9, 2, f16=True)
    assert ws(None, 2) == -lib.E_NULL
    for S in (0, 1, 9):
        assert ws(ctypes.byref(_valid()), S) == -lib.E_DIM
    for field in ("in_lo", "w_lo", "add_hi", "add_lo", "tail_w_hi", "tail_w_lo", "addend", "up_out", "up_depth", "gu_in",
                  "gu_out"):
        x = _valid(); setattr(x.base, field, 16)
        assert ws(ctypes.byref(x), 2) == -lib.E_DIM, field
    for over in (dict(taps=4), dict(dil=2), dict(cout_pad=64), dict(cout_pad=192), dict(out_mode=2), dict(out_mode=4), dict(cin=176),
                 dict(cin=96), dict(rows=0)):
        x = _valid()
        for k, v in over.items():
            setattr(x.base, k, v)
        assert ws(ctypes.byref(x), 2) == -lib.E_DIM, over
    for tiling in (lib.TILING_BM64, lib.TILING_BM256, 8):
        x = _valid(); x.tiling = tiling
        assert ws(ctypes.byref(x), 2) == -lib.E_DIM
    x = _valid(); x.act = 7
    assert ws(ctypes.byref(x), 2) == -lib.E_DIM
    for mode in (0, 1, 3):                                                      # the three output forms are served
        x = _valid(); x.base.out_mode = mode
        assert ws(ctypes.byref(x), 2) == 2 * 330 * 256 * 4
    # the bf16x3 form's query answers as before: out_mode 3 is not its form
    x = _valid(); x.base.in_lo = x.base.w_lo = 16
    assert L.magnet_conv_mfma_splitk_workspace(ctypes.byref(x), 2) == -lib.E_DIM


def test_entry_point_refusals_come_before_a_launch(hip_lib):
    L = hip_lib
    run, sk = L.magnet_conv_mfma_f16d, L.magnet_conv_mfma_f16d_splitk
    need = 2 * 330 * 256 * 4
    assert run(None, None) == lib.E_NULL and sk(None, 2, 16, need, None) == lib.E_NULL
    for field in ("in_lo", "w_lo", "add_hi", "add_lo", "tail_w_hi", "addend", "up_out", "gu_in"):
        x = _valid(); setattr(x.base, field, 16)
        assert run(ctypes.byref(x), None) == lib.E_DIM and sk(ctypes.byref(x), 2, 16, need, None) == lib.E_DIM, field
    for tiling in (lib.TILING_BM64, lib.TILING_BM256):
        x = _valid(); x.tiling = tiling
        assert run(ctypes.byref(x), None) == lib.E_DIM and b"tiling" in L.magnet_last_error()
    for over in (dict(cout_pad=64), dict(out_mode=2), dict(taps=4), dict(dil=2)):
        x = _valid()
        for k, v in over.items():
            setattr(x.base, k, v)
        assert run(ctypes.byref(x), None) == lib.E_DIM, over
    x = _valid(); x.act, x.act_slope, x.base.relu = lib.ACT_LEAKY_RELU, 0.01, 1
    assert run(ctypes.byref(x), None) == lib.E_DIM and b"LeakyReLU" in L.magnet_last_error()
    x = _valid(); x.act, x.act_slope = lib.ACT_LEAKY_RELU, float("nan")
    assert run(ctypes.byref(x), None) == lib.E_DIM
    x = _valid(); x.base.w_hi = 24
    assert run(ctypes.byref(x), None) == lib.E_ALIGN                            # the base checks apply
    x = _valid(); x.base.out_hi = None
    assert run(ctypes.byref(x), None) == lib.E_NULL
    x = _valid()
    assert sk(ctypes.byref(x), 2, None, need, None) == lib.E_NULL
    assert sk(ctypes.byref(x), 2, 24, need, None) == lib.E_ALIGN
    assert sk(ctypes.byref(x), 2, 16, need - 1, None) == lib.E_DIM and b"work_bytes" in L.magnet_last_error()
    for S in (1, 9, 3):
        assert sk(ctypes.byref(x), S, 16, need * 8, None) == lib.E_DIM


def test_lib_conv_mfma_routes():
    t = torch.zeros(1)
    base = dict(in_hi=t, in_lo=None, in_ld=64, cin=64, w_hi=t, w_lo=None, bias=t, taps=9, wp=10, relu=False, rows=100, out_f32=t)
    for f16 in (True, "plane"):                                                 # the two earlier formats still refuse split_k
        with pytest.raises(lib.MagnetError, match="split_k"):
            lib.conv_mfma(**base, f16=f16, split_k=2, work=t)
    for kw in (dict(tail=(t, t, t, 16)), dict(addend=t), dict(add=(t, None, 128)), dict(out_bf16=t), dict(dil=2)):
        with pytest.raises(lib.MagnetError, match="wide"):
            lib.conv_mfma(**base, f16="wide", **kw)
    with pytest.raises(lib.MagnetError, match="f16 must be"):
        lib.conv_mfma(**base, f16="narrow")
    with pytest.raises(lib.MagnetError, match="work"):
        lib.conv_mfma(**base, f16="wide", split_k=2, work=None)
    with pytest.raises(lib.MagnetError, match="fp16 GPU tensor"):
        lib.conv_mfma(**base, f16="wide", leaky=0.01)                           # leaky is accepted on this route; the CPU tensor is not
    with pytest.raises(lib.MagnetError, match="leaky"):
        lib.conv_mfma(**base, f16="plane", leaky=0.01)
