"""FNetMFMA(precision="fp16") / MAGNET(fnet_precision="fp16"), the parts that need no GPU: the refusals at construction, the one-plane
weight packers against the fp32 packers, and the argument checks of magnet_conv_mfma_f16p through the loaded library (codes, not
crashes: every call here is refused before anything is launched)."""
import ctypes

import pytest
import torch

from magnet_amd import fnet, lib
from magnet_amd.planes import fold_bn, pack_s2d, pack_s2d_f16, pack_taps, pack_taps_f16, to_f16_sat
from tests.stubs import StubDNet, make_args, seeded_fnet_state


def _magnet(**kw):
    import warnings
    from magnet_amd.magnet import MAGNET
    args = make_args(D=16, iters=2, dpv_h=64, dpv_w=80, fdim=64, V=2)
    args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MAGNET(args, d_net=StubDNet(0), f_net=fnet.FNET(args), **kw)


def test_refusals_at_construction():
    psm = fnet.PSMNet(feature_dim=64)
    with pytest.raises(lib.MagnetError, match="precision"):
        fnet.FNetMFMA(psm, precision="fp8")
    with pytest.raises(lib.MagnetError, match="fnet_precision"):
        _magnet(fnet_precision="fp16", conv_backend="torch")
    with pytest.raises(lib.MagnetError, match="fnet_precision"):
        _magnet(fnet_precision="fp8")
    # conv_precision stays independent: it is neither implied nor required
    m = _magnet(fnet_precision="fp16")
    assert m.fnet_precision == "fp16" and m.conv_precision == "bf16x3"
    assert m._fnet_runner().precision == "fp16"


def test_defaults_construct_what_they_construct_today():
    psm = fnet.PSMNet(feature_dim=64)
    r = fnet.FNetMFMA(psm)
    assert r.precision == "bf16x3" and r._f16 is False
    assert fnet.FNetMFMA(psm, precision="bf16x3").precision == "bf16x3"
    m = _magnet()
    assert m.fnet_precision == "bf16x3" and m._fnet_runner().precision == "bf16x3"
    # the default pack is the split-bf16 one: (hi, lo, bias, cout) with bf16 planes
    P = r.packed(torch.device("cpu"))
    hi, lo, bias, cout = P["layer1.0.conv1"]
    assert hi.dtype == lo.dtype == torch.bfloat16 and bias.dtype == torch.float32 and cout == 32


def test_f16_pack_is_one_plane_per_layer_and_cached_per_precision():
    psm = seeded_fnet_state(fnet.PSMNet(feature_dim=64), seed=3).eval()
    r16, r = fnet.FNetMFMA(psm, precision="fp16"), fnet.FNetMFMA(psm)
    cpu = torch.device("cpu")
    P16, P = r16.packed(cpu), r.packed(cpu)
    assert set(P16) == set(P) and r16.packed(cpu) is P16
    for name in P:
        if name == "stem":
            assert torch.equal(P16[name][0], P[name][0]) and torch.equal(P16[name][1], P[name][1])      # the stem stays fp32
            continue
        w16, none, b16, cout = P16[name]
        hi, lo, b, cout0 = P[name]
        assert none is None and w16.dtype == torch.float16 and w16.shape == hi.shape and cout == cout0 and torch.equal(b16, b)
    # switching the precision repacks (one cache entry per precision), and switching back finds the first pack again
    r16.precision, r16._f16 = "bf16x3", False
    Pb = r16.packed(cpu)
    assert Pb is not P16 and Pb["layer1.0.conv1"][0].dtype == torch.bfloat16
    r16.precision, r16._f16 = "fp16", "plane"
    assert r16.packed(cpu) is P16
    with pytest.raises(lib.MagnetError, match="feature_dim"):
        fnet.FNetMFMA(fnet.PSMNet(feature_dim=16), precision="fp16").packed(cpu)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("s2d", [False, True], ids=["taps", "s2d"])
def test_f16_packers_equal_f16_of_the_fp32_packers(s2d):
    """pack_taps_f16 / pack_s2d_f16 of a BatchNorm-folded layer against the fp32 packers' planes, for seeded weights with one weight at
    the clamp (7e4 -> 65504), one below the denormal range (1e-8 -> 0: under half the smallest denormal 2^-25) and one kept denormal.

    The fold happens in fp32 and each weight is rounded ONCE, so the exact statement is: the plane == to_f16_sat of the fp32 weights in
    the fp32 packer's layout, bit for bit (checked first, on the layout the fp32 packer itself produces: same positions, same zeros).
    Against to_f16_sat(hi + lo) bit-equality cannot hold everywhere: hi + lo is w rounded to 16 significant bits, so f16(hi + lo) is w
    rounded TWICE and lands on the other neighbour whenever an fp16 rounding tie lies between w and hi + lo (expected for a fraction
    ~2^-6 of random mantissas; 94 of 32 768 elements of the s2d plane here).  So every element is bit-equal, or the two results are
    adjacent fp16 values whose midpoint (the tie) lies between w and hi + lo, and wherever hi + lo == w they are bit-equal."""
    psm = seeded_fnet_state(fnet.PSMNet(feature_dim=64), seed=7).eval()
    unit = psm.layer2[0]
    conv, bn = unit.conv1[0]
    w = fold_bn(conv, bn)[0].float()                                 # (64, 32, 3, 3), fp32 as FNetMFMA._pack folds it
    w[3, 5, 1, 1] = 7e4
    w[4, 6, 0, 2] = 1e-8
    w[5, 7, 2, 0] = -7e4
    w[6, 8, 1, 2] = 3e-6                                             # an fp16 denormal that survives
    got = (pack_s2d_f16 if s2d else pack_taps_f16)(w)
    hi, lo = (pack_s2d if s2d else pack_taps)(w)
    assert got.dtype == torch.float16 and got.shape == hi.shape and got.is_contiguous()
    from magnet_amd.planes import s2d_matrix
    w32 = s2d_matrix(w) if s2d else w.permute(2, 3, 0, 1).reshape(9, 64, 32)          # the fp32 values in the packer's layout
    assert torch.equal(_bits(got), _bits(to_f16_sat(w32))), "not the single saturating rounding of the fp32 weight"
    s = hi.float() + lo.float()                                                       # exact in fp32 (16 significant bits)
    exp = to_f16_sat(s)
    same = _bits(got) == _bits(exp)
    assert bool(same[s == w32].all()), "differs from f16(hi + lo) where hi + lo IS the fp32 weight"
    d = ~same
    print(f"[f16 packers {'s2d' if s2d else 'taps'}] {int(d.sum())} of {d.numel()} differ from f16(hi + lo) by the double rounding")
    if bool(d.any()):
        g, e, wv, sv = got[d].double(), exp[d].double(), w32[d].double(), s[d].double()
        assert bool(((_bits(got)[d].int() - _bits(exp)[d].int()).abs() == 1).all()), "not adjacent fp16 values"
        tie = (g + e) / 2
        assert bool(((torch.minimum(wv, sv) <= tie) & (tie <= torch.maximum(wv, sv))).all()), "no rounding tie between w and hi + lo"
    flat = got.float().flatten()
    assert flat.max().item() == 65504.0 and flat.min().item() == -65504.0
    assert bool(torch.isfinite(got.float()).all())
    if not s2d:
        assert got[1 * 3 + 1, 3, 5].item() == 65504.0 and got[0 * 3 + 2, 4, 6].item() == 0.0 and got[2 * 3 + 0, 5, 7].item() == -65504.0
        d = got[1 * 3 + 2, 6, 8].float().item()
        assert d != 0.0 and abs(d - 3e-6) <= 2.0 ** -25                  # kept as a denormal: absolute rounding 2^-25


def _conv_args(**over):
    """A magnet_conv_mfma_f16p argument block that passes every check (no launch happens in this file: each call below breaks one)."""
    a = lib.MagnetConvArgs()
    a.in_hi = a.w_hi = a.bias = a.out_hi = 16
    a.rows, a.cin, a.cout_pad, a.taps, a.wp, a.out_mode = 128, 64, 64, 9, 10, 3
    tiling = over.pop("tiling", 0)
    for k, v in over.items():
        setattr(a, k, v)
    return lib.MagnetConvExArgs(base=a, tiling=tiling)


def test_f16p_argument_errors_are_codes_not_crashes(hip_lib):
    f = hip_lib.magnet_conv_mfma_f16p
    assert f(None, None) == lib.E_NULL
    for name, over in (("in_lo", dict(in_lo=16)), ("w_lo", dict(w_lo=16)), ("add_lo", dict(add_hi=16, add_lo=16)),
                       ("add_lo alone", dict(add_lo=16)),
                       ("fused tail", dict(tail_w_hi=16, tail_w_lo=16, tail_bias=16, tail_cout_pad=16, out_f32=16, cout_pad=128)),
                       ("addend", dict(addend=16)), ("BM64", dict(tiling=lib.TILING_BM64)), ("BM256", dict(tiling=lib.TILING_BM256)),
                       ("out_mode 0", dict(out_mode=0, out_lo=16)), ("out_mode 4", dict(out_mode=4)),
                       ("cout_pad 16", dict(cout_pad=16)), ("cout_pad 144", dict(cout_pad=144)), ("cout_pad 256", dict(cout_pad=256)),
                       ("taps 5", dict(taps=5)), ("cin 48", dict(cin=48))):
        assert f(ctypes.byref(_conv_args(**over)), None) == lib.E_DIM, name
        assert hip_lib.magnet_last_error(), name
    x = _conv_args()
    x.act = lib.ACT_LEAKY_RELU
    assert f(ctypes.byref(x), None) == lib.E_DIM
    assert f(ctypes.byref(_conv_args(in_hi=0)), None) == lib.E_NULL
    assert f(ctypes.byref(_conv_args(out_hi=0)), None) == lib.E_NULL
    assert f(ctypes.byref(_conv_args(add_hi=24)), None) == lib.E_ALIGN
    # the other entry points keep refusing the new output form
    assert hip_lib.magnet_conv_mfma_ex(ctypes.byref(_conv_args(in_lo=16, w_lo=16)), None) == lib.E_DIM
    b = _conv_args(in_lo=16, w_lo=16).base
    assert hip_lib.magnet_conv_mfma(ctypes.byref(b), None) == lib.E_DIM and b"out_mode" in hip_lib.magnet_last_error()
    assert hip_lib.magnet_conv_mfma_f16(ctypes.byref(_conv_args(cout_pad=128)), None) == lib.E_DIM


def test_f16_small_kernel_argument_errors(hip_lib):
    assert hip_lib.magnet_fnet_stem_f16(None, 16, 16, 16, 1, 8, 8, None) == lib.E_NULL
    assert hip_lib.magnet_fnet_stem_f16(16, 16, 16, 16, 1, 1, 8, None) == lib.E_DIM
    assert hip_lib.magnet_fnet_stem_f16(16, 16, 16, 24, 1, 8, 8, None) == lib.E_ALIGN
    assert hip_lib.magnet_space_to_depth_f16(16, 16, 1, 12, 4, 4, 2, None) == lib.E_DIM            # C % 8
    assert hip_lib.magnet_space_to_depth_f16(16, None, 1, 32, 4, 4, 2, None) == lib.E_NULL
    assert hip_lib.magnet_avgpool_cl_f16(16, 320, 1, 8, 8, 2, 16, 128, 16, None) == lib.E_DIM       # window larger than the map
    assert hip_lib.magnet_upsample_bilinear_cl_f16(16, 32, 1, 2, 32, 24, 320, 1, 8, 8, 2, None) == lib.E_ALIGN
    assert hip_lib.magnet_upsample_bilinear_cl_f16(16, 32, 1, 2, 32, 16, 324, 1, 8, 8, 2, None) == lib.E_DIM   # out_ld % 8


def test_lib_conv_mfma_plane_route_type_checks():
    """The Python route refuses wrong tensors before it reaches the library (CPU tensors here: no GPU is needed to be refused)."""
    x = torch.zeros((128, 64), dtype=torch.float16)
    w = torch.zeros((9, 64, 64), dtype=torch.float16)
    b = torch.zeros(64)
    with pytest.raises(lib.MagnetError, match="fp16 GPU tensor"):
        lib.conv_mfma(x, None, 64, 64, w, None, b, 9, 10, True, 128, out_hi=x, f16="plane")
    with pytest.raises(lib.MagnetError, match="one fp16 plane"):
        lib.conv_mfma(x, x, 64, 64, w, None, b, 9, 10, True, 128, out_hi=x, f16="plane")
    with pytest.raises(lib.MagnetError, match="out_lo"):
        lib.conv_mfma(x, None, 64, 64, w, None, b, 9, 10, True, 128, out_hi=x, out_lo=x, f16="plane")
    with pytest.raises(lib.MagnetError, match="f16 must be"):
        lib.conv_mfma(x, None, 64, 64, w, None, b, 9, 10, True, 128, out_hi=x, f16="planes")
