"""The split-K route's host side: the "auto" rule (magnet_amd.dnet.split_factor), the argument errors of magnet_conv_mfma_splitk and
its workspace query as codes, and the split_k validation of DNetMFMA, DNET and MAGNET.  No GPU needed: every refusal comes before a
launch."""
import ctypes

import pytest
import torch

from magnet_amd import dnet, lib
from magnet_amd.dnet import DNET, DNetMFMA, split_factor
from magnet_amd.magnet import MAGNET
from magnet_amd.standin import StandinEncoder, StubFNet, make_args, make_dnet, make_dnet_args

# (layer, stride of its grid, 32-channel chunks of its input, 128-channel N tiles)
LAYERS = (("conv2", 32, 64, 16), ("up1.0", 16, 70, 8), ("up1.1", 16, 32, 8), ("up2.0", 8, 34, 4), ("up2.1", 8, 16, 4),
          ("up3.0", 4, 18, 2), ("up3.1", 4, 8, 2))


def launches(N, H, W):
    """(layer, row tiles, N tiles, chunks) of the decoder's plain launches for N images of H x W (zero-bordered grids, 128-row tiles)."""
    out = []
    for name, s, chunks, nt in LAYERS:
        rows = N * (H // s + 2) * (W // s + 2)
        out.append((name, (rows + 127) // 128, nt, chunks))
    return out


def test_tile_arithmetic_of_the_helper():
    assert [(r, n) for _, r, n, _ in launches(1, 480, 640)] == [(3, 16), (11, 8), (11, 8), (40, 4), (40, 4), (155, 2), (155, 2)]
    assert [r * n for _, r, n, _ in launches(1, 352, 1216)] == [80, 120, 120, 224, 224, 432, 432]


def test_split_factor_is_one_when_the_chip_is_full():
    for _, r, n, c in launches(20, 480, 640):
        assert r * n >= dnet.SPLIT_CUS and split_factor(r, n, c) == 1
    assert split_factor(dnet.SPLIT_CUS, 1, 64) == 1 and split_factor(1, dnet.SPLIT_CUS, 64) == 1


def test_split_factor_properties():
    assert dnet.SPLIT_AUTO_MIN_CHUNKS >= lib.SPLITK_MIN_CHUNKS
    for chunks in (1, 2, 3, 8, 16, 18, 32, 34, 64, 70, 1000):
        prev = lib.SPLITK_MAX
        for wg in range(1, 600):
            s = split_factor(wg, 1, chunks)
            assert 1 <= s <= lib.SPLITK_MAX
            assert s <= prev                                           # non-increasing in the workgroup count
            prev = s
            assert s == split_factor(1, wg, chunks)                    # depends on the product only
            if s > 1:
                assert chunks // s >= lib.SPLITK_MIN_CHUNKS           # every split gets floor(chunks / s) chunks or one more
                assert wg * s <= dnet.SPLIT_SLOTS and wg < dnet.SPLIT_CUS
                assert wg * s <= dnet.SPLIT_CUS or s == 2              # one workgroup per CU, or the smallest split
                assert chunks // s >= dnet.SPLIT_AUTO_MIN_CHUNKS
    with pytest.raises(lib.MagnetError):
        split_factor(0, 1, 8)


def test_split_factor_for_one_image():
    """The factors "auto" takes at the two shapes of the sweep (profiles/splitk/NOTES.md)."""
    got = {name: split_factor(r, n, c) for name, r, n, c in launches(1, 480, 640)}
    assert got == {"conv2": 5, "up1.0": 2, "up1.1": 2, "up2.0": 2, "up2.1": 2, "up3.0": 1, "up3.1": 1}
    got = {name: split_factor(r, n, c) for name, r, n, c in launches(1, 352, 1216)}
    assert got == {"conv2": 3, "up1.0": 2, "up1.1": 2, "up2.0": 2, "up2.1": 2, "up3.0": 1, "up3.1": 1}


def _valid():
    x = lib.MagnetConvExArgs()
    c = x.base
    c.in_hi = c.in_lo = c.w_hi = c.w_lo = c.bias = c.out_hi = c.out_lo = c.out_f32 = 16
    c.rows, c.cin, c.cout_pad, c.taps, c.wp, c.out_mode = 510, 160, 256, 9, 17, 1
    return x


def test_splitk_argument_errors_are_codes(hip_lib):
    L = hip_lib
    ws, run = L.magnet_conv_mfma_splitk_workspace, L.magnet_conv_mfma_splitk
    x = _valid()
    assert ws(ctypes.byref(x), 2) == 2 * 510 * 256 * 4
    assert lib.conv_mfma_splitk_workspace(510, 160, 256, 9, 2) == 2 * 510 * 256 * 4
    assert ws(None, 2) == -lib.E_NULL and run(None, 2, 16, 1 << 30, None) == lib.E_NULL
    big = 1 << 30

    def both(x, s, code, word=None):
        assert ws(ctypes.byref(x), s) == -code
        assert run(ctypes.byref(x), s, 16, big, None) == code
        if word:
            assert word in L.magnet_last_error()

    for s in (-1, 0, 1, 9):
        both(x, s, lib.E_DIM, b"split_k")
    both(x, 3, lib.E_DIM, b"chunks")                                   # 5 chunks: 3 splits would leave one of them a single chunk
    x.base.cin = 512
    assert ws(ctypes.byref(x), 8) == 8 * 510 * 256 * 4                 # 16 chunks: 2 each
    x = _valid(); x.base.cout_pad = 144
    both(x, 2, lib.E_DIM, b"cout_pad")
    x = _valid(); x.base.cout_pad = 64
    both(x, 2, lib.E_DIM, b"cout_pad")
    x = _valid(); x.base.taps = 4
    both(x, 2, lib.E_DIM, b"taps")
    x = _valid(); x.base.cin = 176
    both(x, 2, lib.E_DIM)
    x = _valid(); x.base.rows = 0
    both(x, 2, lib.E_DIM)
    for field in ("tail_w_hi", "addend", "add_hi", "add_lo", "up_out", "gu_in"):
        x = _valid(); setattr(x.base, field, 16)
        both(x, 2, lib.E_DIM, b"plain bf16x3 layer only")
    for tiling in (lib.TILING_BM64, lib.TILING_BM256, 8):
        x = _valid(); x.tiling = tiling
        both(x, 2, lib.E_DIM, b"tiling")
    for mode in (2, 3, -1):
        x = _valid(); x.base.out_mode = mode
        both(x, 2, lib.E_DIM, b"out_mode")
    # the workspace itself
    x = _valid()
    need = 2 * 510 * 256 * 4
    assert run(ctypes.byref(x), 2, None, need, None) == lib.E_NULL
    assert run(ctypes.byref(x), 2, 24, need, None) == lib.E_ALIGN
    assert run(ctypes.byref(x), 2, 16, need - 1, None) == lib.E_DIM and b"work_bytes" in L.magnet_last_error()
    # the activation mode and the base checks apply as in magnet_conv_mfma_ex
    x.act = 7
    assert run(ctypes.byref(x), 2, 16, need, None) == lib.E_DIM and b"act" in L.magnet_last_error()
    x.act, x.act_slope, x.base.relu = lib.ACT_LEAKY_RELU, 0.01, 1
    assert run(ctypes.byref(x), 2, 16, need, None) == lib.E_DIM and b"LeakyReLU" in L.magnet_last_error()
    x = _valid(); x.base.in_lo = None
    assert run(ctypes.byref(x), 2, 16, need, None) == lib.E_NULL
    x = _valid(); x.base.w_hi = 24
    assert run(ctypes.byref(x), 2, 16, need, None) == lib.E_ALIGN
    x = _valid(); x.base.wp = 0
    assert run(ctypes.byref(x), 2, 16, need, None) == lib.E_DIM


def test_lib_conv_mfma_refuses_split_k_with_other_forms():
    t = torch.zeros(1)
    base = dict(in_hi=t, in_lo=t, in_ld=64, cin=64, w_hi=t, w_lo=t, bias=t, taps=9, wp=10, relu=False, rows=100, out_f32=t)
    for kw in (dict(f16=True), dict(f16="plane"), dict(tail=(t, t, t, 16)), dict(addend=t), dict(add=(t, t, 128))):
        with pytest.raises(lib.MagnetError, match="split_k"):
            lib.conv_mfma(**base, split_k=2, work=t, **kw)
    with pytest.raises(lib.MagnetError, match="work"):
        lib.conv_mfma(**base, split_k=2, work=None)
    with pytest.raises(lib.MagnetError, match="work goes with split_k"):
        lib.conv_mfma(**base, work=t)


def test_runner_split_k_validation():
    dec = make_dnet().d_net.decoder
    assert DNetMFMA(dec).split_k == 0
    assert DNetMFMA(dec, split_k="auto").split_k == "auto"
    forced = {"conv2": 2, "up3.1": 3, "up1.0": 1}
    assert DNetMFMA(dec, split_k=forced).split_k == forced
    for bad in ("on", 1, 2, True, None, 0.0, {"conv3": 2}, {"conv2": 0}, {"conv2": 9}, {"conv2": True}, {"up1.0": 2.0}):
        with pytest.raises(lib.MagnetError, match="split_k"):
            DNetMFMA(dec, split_k=bad)


def test_dnet_and_magnet_split_k_validation():
    assert DNET(make_dnet_args(), StandinEncoder(), backend="hip")._runner.split_k == 0
    assert DNET(make_dnet_args(), StandinEncoder(), backend="hip", split_k="auto")._runner.split_k == "auto"
    assert DNET(make_dnet_args(), StandinEncoder(), dnet=True, backend="hip", split_k={"up2.0": 2})._runner.split_k == {"up2.0": 2}
    with pytest.raises(lib.MagnetError, match="backend='hip'"):
        DNET(make_dnet_args(), StandinEncoder(), split_k="auto")
    with pytest.raises(lib.MagnetError, match="split_k"):
        DNET(make_dnet_args(), StandinEncoder(), backend="hip", split_k="yes")
    d = make_dnet()
    m = MAGNET(make_args(), d_net=d, f_net=StubFNet(), dnet_backend="hip")
    assert m.dnet_split_k == 0 and m._dnet.split_k == 0
    m = MAGNET(make_args(), d_net=d, f_net=StubFNet(), dnet_backend="hip", dnet_split_k="auto")
    assert m.dnet_split_k == "auto" and m._dnet.split_k == "auto"
    with pytest.raises(lib.MagnetError, match="dnet_backend='hip'"):
        MAGNET(make_args(), d_net=d, f_net=StubFNet(), dnet_split_k="auto")
    with pytest.raises(lib.MagnetError, match="split_k"):
        MAGNET(make_args(), d_net=d, f_net=StubFNet(), dnet_backend="hip", dnet_split_k=3)
