"""conv_precision: the constructor's rules, and the fp64 / numpy restatement of the single-plane fp16 format's conversion
(include/magnet_hip.h) that tests/test_gpu_conv_f16.py uses as its bit-exact reference.  No GPU.

The conversion: round to nearest even onto the fp16 grid (quantum 2^(e - 10) for 2^e <= |x| < 2^(e + 1), e >= -14; 2^-24 below
2^-14), after clamping to [-65504, 65504] — so a magnitude that would round above 65504 (from 65520 on, +-Inf included) becomes
+-65504; NaN stays NaN; the sign of zero, and of a value that rounds to zero, is kept.
"""
import warnings

import numpy as np
import pytest
import torch


def f16_sat_bits(x) -> np.ndarray:
    """uint16 bit patterns of the format's conversion of fp32 values, worked in fp64 without numpy's own fp16 cast: every fp32 value,
    its power-of-two quantum and their quotient are exact in fp64, and np.rint rounds ties to even."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    nan = np.isnan(x)
    c = np.clip(np.where(nan, 0.0, x), -65504.0, 65504.0)
    mag = np.abs(c)
    e = np.floor(np.log2(np.where(mag > 0, mag, 1.0)))
    e = np.where(mag >= 2.0 ** e, e, e - 1)                      # guard log2 rounding up at a binade's top (it does not for fp32 inputs)
    q = 2.0 ** (np.maximum(e, -14.0) - 10.0)
    n = np.rint(mag / q)                                         # 0 .. 2048 quanta; 2048 = the next binade's 1024
    r = n * q                                                    # <= 65504: 65504 = 2047 * 32 is the clamp's own bound
    assert (r <= 65504.0).all()
    # r is on the fp16 grid: assemble its bits.  r < 2^-14: denormal, bits = n.  Else exponent field e' + 15, mantissa r / 2^(e' - 10) - 1024
    e2 = np.floor(np.log2(np.where(r > 0, r, 1.0)))
    norm = r >= 2.0 ** -14
    bits = np.where(norm, ((e2 + 15).astype(np.int64) << 10) + (r / 2.0 ** (e2 - 10.0)).astype(np.int64) - 1024, n.astype(np.int64))
    bits = np.where(r == 0, 0, bits) | (np.signbit(c).astype(np.int64) << 15)
    return np.where(nan, 0x7E00, bits).astype(np.uint16)


def f16_is_nan(bits) -> np.ndarray:
    bits = np.asarray(bits).astype(np.int64)
    return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)


def assert_f16_bits_equal(name, got_bits, exp_bits):
    """Bit for bit, except that any NaN matches any NaN (the kernels keep a payload)."""
    got_bits, exp_bits = np.asarray(got_bits), np.asarray(exp_bits)
    bad = (got_bits != exp_bits) & ~(f16_is_nan(got_bits) & f16_is_nan(exp_bits))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: fp16 bits differ at {i}: got {int(got_bits[i]):#06x}, expected {int(exp_bits[i]):#06x} ({int(bad.sum())} elements)")


def planes_sum_f32(hi_bits, lo_bits) -> np.ndarray:
    """hi + lo of bf16 bit patterns (uint16), the sum formed in fp32 — what magnet_planes_to_f16 converts."""
    hi = (np.asarray(hi_bits).astype(np.uint32) << 16).view(np.float32)
    lo = (np.asarray(lo_bits).astype(np.uint32) << 16).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (hi + lo).astype(np.float32)


# (value, expected bits); NaN is checked apart
EDGES = [
    (65504.0, 0x7BFF), (-65504.0, 0xFBFF),
    (65519.996, 0x7BFF),                          # the largest fp32 below 65520 is nearer to 65504 than to 65536
    (65520.0, 0x7BFF), (-65520.0, 0xFBFF),        # a tie that RNE would take to Inf: clamped
    (1e30, 0x7BFF), (float("inf"), 0x7BFF), (float("-inf"), 0xFBFF),
    (2.0 ** -14, 0x0400), (2.0 ** -14 - 2.0 ** -25, 0x0400),   # smallest normal; just below it, a tie to the even 1024 quanta
    (2.0 ** -24, 0x0001),
    (-(2.0 ** -24), 0x8001),
    (2.0 ** -25, 0x0000), (-(2.0 ** -25), 0x8000),             # ties to even: zero, with its sign
    (3 * 2.0 ** -25, 0x0002), (2.0 ** -25 * 1.0000001, 0x0001),
    (0.0, 0x0000), (-0.0, 0x8000), (1e-30, 0x0000), (-1e-30, 0x8000),
    (1.0, 0x3C00), (1.0 + 2.0 ** -11, 0x3C00), (1.0 + 3 * 2.0 ** -11, 0x3C02), (2049.0, 0x6800), (2051.0, 0x6802),
]
EDGE_VALUES = np.array([v for v, _ in EDGES] + [float("nan")], dtype=np.float32)


def test_edge_values_of_the_conversion():
    got = f16_sat_bits(EDGE_VALUES)
    for (v, want), g in zip(EDGES, got[:-1]):
        assert int(g) == want, f"{v!r}: {int(g):#06x}, expected {want:#06x}"
    assert f16_is_nan(got[-1:]).all()
    assert np.float32(65519.996) < np.float32(65520.0)


def test_restatement_agrees_with_numpy_and_torch_casts_inside_the_domain():
    """Where no clamp applies (|x| < 65520) the format is plain IEEE round-to-nearest-even: the restatement, numpy's cast and
    planes.to_f16_sat must agree bit for bit — on random values over every fp16 binade, the denormal range and exact ties."""
    from magnet_amd.planes import to_f16_sat
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * 2.0 ** rng.integers(-30, 16, 200000)).astype(np.float32)
    ties = (rng.integers(0, 2048, 4000) + 0.5) * 2.0 ** rng.integers(-24, 5, 4000)
    x = np.concatenate([x, ties.astype(np.float32), -ties.astype(np.float32), EDGE_VALUES])
    inside = ~(np.abs(x) >= 65520)
    ours = f16_sat_bits(x)
    with warnings.catch_warnings(), np.errstate(over="ignore"):
        warnings.simplefilter("ignore")
        theirs = x.astype(np.float16).view(np.uint16)
    assert_f16_bits_equal("numpy cast", ours[inside], theirs[inside])
    assert_f16_bits_equal("planes.to_f16_sat", to_f16_sat(torch.from_numpy(x)).view(torch.int16).numpy().view(np.uint16), ours)


def test_pack_taps_f16_layout_and_padding():
    from magnet_amd.planes import pack_taps, pack_taps_f16
    w = torch.randn(16, 5, 3, 3, generator=torch.Generator().manual_seed(1))
    w[0, 0, 0, 0] = 1e9
    p = pack_taps_f16(w, 32)
    assert p.dtype == torch.float16 and tuple(p.shape) == (9, 16, 32) and p.is_contiguous()
    assert bool((p[:, :, 5:] == 0).all()) and float(p[0, 0, 0]) == 65504.0
    hi, _ = pack_taps(w, 32)
    assert tuple(hi.shape) == tuple(p.shape)
    want = f16_sat_bits(w.permute(2, 3, 0, 1).reshape(9, 16, 5).numpy())
    assert_f16_bits_equal("pack_taps_f16", p[:, :, :5].contiguous().view(torch.int16).numpy().view(np.uint16), want)


def _model(**kw):
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import StubDNet, StubFNet, make_args
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MAGNET(make_args(D=8, iters=2, dpv_h=24, dpv_w=32), d_net=StubDNet(1), f_net=StubFNet(2, fdim=16), **kw)


def test_constructor_takes_conv_precision_fp16():
    """On a tree without the mode this is a TypeError (unexpected keyword argument)."""
    m = _model(conv_precision="fp16")
    assert m.conv_precision == "fp16" and m.conv_backend == "mfma"


def test_constructor_rules():
    from magnet_amd import lib
    assert _model().conv_precision == "bf16x3"                                  # the default
    assert _model(conv_precision="bf16x3", conv_backend="torch").conv_precision == "bf16x3"
    with pytest.raises(lib.MagnetError, match="conv_precision must be"):
        _model(conv_precision="bf16")
    with pytest.raises(lib.MagnetError, match="conv_precision must be"):
        _model(conv_precision="fp32")
    with pytest.raises(lib.MagnetError, match="needs conv_backend='mfma'"):
        _model(conv_precision="fp16", conv_backend="torch")
    for tb in ("torch", "hip"):                                                 # the training path is not the mode's business
        assert _model(conv_precision="fp16", train_backend=tb).train_backend == tb


def test_small_tiles_with_f16_is_an_error():
    from magnet_amd import lib
    from magnet_amd.convnet import ConvStackMFMA
    import torch.nn as nn
    seq = nn.Sequential(nn.Conv2d(32, 128, 3, padding=1), nn.ReLU(), nn.Conv2d(128, 128, 1), nn.ReLU(), nn.Conv2d(128, 128, 1), nn.ReLU(),
                        nn.Conv2d(128, 2, 1))
    st = ConvStackMFMA(seq)
    st.small_tiles = True
    x = torch.zeros((48, 32), dtype=torch.float16)
    with pytest.raises(lib.MagnetError, match="no 64-row tile form"):
        st.run(x, None, 32, 48, 8, {}, f16=True)
    with pytest.raises(lib.MagnetError, match="no 64-row tile form"):
        st.run_invariant(x, None, 32, 48, 8, {}, 8, 0, f16=True)
