"""magnet_conv_mfma_nchw and the step's route to it, without a GPU.

The entry point serves one form (include/magnet_hip.h) and refuses everything else with a code before any launch: the arguments
below carry fake device pointers, so a call that got as far as a launch would not return a MAGNET_E_* code — and the refusal tests
skip themselves where a device is visible, as tests/test_conv_refusals_host.py does.  x_d3_route() is the one place that decides
whether MAGNET._refine_mfma skips x_d3's pack pass; it is host arithmetic."""
import ctypes

import pytest

PTR = 1 << 20                                     # a 16-byte-aligned fake device address


def _args(B=5, h=32, w=14, kind="gnet", tiling=None):
    """Arguments the entry point would launch: (5, 32, 14) tiles per image on the 256-row kernel (tests/test_gpu_conv_image_tiles.py)."""
    from magnet_amd import lib
    n = lib.MagnetConvNchwArgs()
    b = n.ex.base
    b.in_hi = b.in_lo = b.w_hi = b.w_lo = b.bias = b.tail_w_hi = b.tail_w_lo = b.tail_bias = PTR
    b.rows, b.wp, b.taps, b.cout_pad, b.relu, b.out_mode = B * (h + 2) * (w + 2), w + 2, 9, 128, 1, 1
    b.up_B, b.up_h, b.up_w = B, h, w
    if kind == "gnet":
        b.cin = b.in_ld = 320
        b.tail_cout_pad, b.gu_in, b.gu_out = 16, PTR, 2 * PTR
        n.src_c0, n.src_C = 64, 256
    else:
        b.cin = b.in_ld = 256
        b.tail_cout_pad, b.up_depth, b.up_out, b.up_npred = 144, PTR, 2 * PTR, 1
        b.in_hi = b.in_lo = None
        n.src_c0, n.src_C = 0, 256
    n.src = 3 * PTR
    n.ex.tiling = lib.TILING_BM256 if tiling is None else tiling
    return n


def _no_device(hip_lib):
    if hip_lib.magnet_device_count() != 0:
        pytest.skip("a GPU is visible: a wrongly accepted argument set would launch on fake pointers")


def _refused(hip_lib, n, code, word):
    rc = hip_lib.magnet_conv_mfma_nchw(ctypes.byref(n), None)
    msg = hip_lib.magnet_last_error().decode()
    assert rc == code and word in msg, (rc, msg)


@pytest.mark.parametrize("kind", ["gnet", "mask"])
def test_refusals_are_codes_before_any_launch(hip_lib, kind):
    from magnet_amd import lib
    _no_device(hip_lib)
    assert hip_lib.magnet_conv_mfma_nchw(None, None) == lib.E_NULL
    assert lib.conv_row_tiles(2, 40, 16, 256)[1] == 0 and lib.conv_row_tiles(5, 32, 16, 256)[1] == 2
    _refused(hip_lib, _args(2, 40, 14, kind), lib.E_DIM, "per-image tiling")             # flat tiling launches no more tiles
    _refused(hip_lib, _args(kind=kind, tiling=lib.TILING_BM256 | lib.TILING_FLAT), lib.E_DIM, "tiling=")
    _refused(hip_lib, _args(kind=kind, tiling=lib.TILING_BM64), lib.E_DIM, "tiling=")
    _refused(hip_lib, _args(kind=kind, tiling=0), lib.E_DIM, "256-row kernel")            # 2 720 rows: the 128-row kernel's
    n = _args(kind=kind); n.ex.base.addend = PTR
    _refused(hip_lib, n, lib.E_DIM, "no addend")
    n = _args(kind=kind); n.src_c0, n.src_C = 48, n.ex.base.cin - 48
    _refused(hip_lib, n, lib.E_DIM, "src_c0=48")
    n = _args(kind=kind); n.src_C = 224
    _refused(hip_lib, n, lib.E_DIM, "src_c0 + src_C == cin")
    n = _args(kind=kind); n.src = 3 * PTR + 4
    _refused(hip_lib, n, lib.E_ALIGN, "16-byte aligned")
    n = _args(kind=kind); n.src = None
    _refused(hip_lib, n, lib.E_NULL, "src is NULL")
    n = _args(kind=kind); n.ex.act = lib.ACT_LEAKY_RELU
    _refused(hip_lib, n, lib.E_DIM, "act=1")
    n = _args(kind=kind); n.ex.base.dil = 2
    _refused(hip_lib, n, lib.E_DIM, "no dilation")
    n = _args(kind=kind); n.ex.base.tail_cout_pad = 128                                    # a tail without Gaussian update / upsampling
    _refused(hip_lib, n, lib.E_DIM, "fused tail")
    n = _args(kind=kind); n.ex.base.up_h = 31                                              # geometry that does not describe rows
    _refused(hip_lib, n, lib.E_DIM, "do not describe")


def test_planes_are_required_only_below_src_c0(hip_lib):
    from magnet_amd import lib
    _no_device(hip_lib)
    n = _args(kind="gnet"); n.ex.base.in_lo = None
    _refused(hip_lib, n, lib.E_NULL, "NULL input pointer")


FLAGSHIP = dict(x_d3_is_tensor=True, aligned16=True, source="auto", conv_precision="bf16x3", fuse_conv_tail=True, fuse_upsample=True,
                can_fuse_gauss=True, can_fuse_upsample=True, n_iter=1, hoist_invariant=True, downsample_ratio=4, overlap_pack=False,
                overlap_mask_head=False, B=64, h=120, w=160)


def test_route_takes_the_flagship_step_and_nothing_it_does_not_serve(hip_lib):
    from magnet_amd import lib
    from magnet_amd.magnet import x_d3_route
    assert x_d3_route(**FLAGSHIP) == "nchw"
    assert x_d3_route(**{**FLAGSHIP, "n_iter": 3, "hoist_invariant": False}) == "nchw"    # every iteration reads x_d3 in place
    for change in (dict(n_iter=3), dict(conv_precision="fp16"), dict(fuse_conv_tail=False), dict(fuse_upsample=False),
                   dict(x_d3_is_tensor=False), dict(B=2, h=15, w=32), dict(B=3), dict(source="pack"), dict(aligned16=False),
                   dict(can_fuse_gauss=False), dict(can_fuse_upsample=False), dict(downsample_ratio=8), dict(overlap_pack=True),
                   dict(overlap_mask_head=True), dict(n_iter=0), dict(B=64, h=40, w=14), dict(small_tiles=True)):
        assert x_d3_route(**{**FLAGSHIP, **change}) == "pack", change
    # B = 3 frames of 120 x 160 are 59 292 rows: the library's own choice there is the 128-row kernel
    assert 3 * 122 * 162 < 65536 <= 4 * 122 * 162 and x_d3_route(**{**FLAGSHIP, "B": 4}) == "nchw"
    # stacks told to take the 256-row kernel (ConvStackMFMA.tile_256, the GPU tests) lift the row threshold, not the tiling rule
    assert x_d3_route(**{**FLAGSHIP, "B": 2, "h": 15, "w": 32, "tile_256": True}) == "nchw"
    assert x_d3_route(**{**FLAGSHIP, "B": 2, "h": 40, "w": 14, "tile_256": True}) == "pack"
    with pytest.raises(lib.MagnetError):
        x_d3_route(**{**FLAGSHIP, "source": "nchw"})


def test_magnet_defaults_to_auto():
    from magnet_amd.magnet import MAGNET
    from magnet_amd.standin import StubDNet, StubFNet, make_args
    m = MAGNET(make_args(D=8, iters=1, dpv_h=24, dpv_w=32), d_net=StubDNet(1), f_net=StubFNet(2, fdim=16))
    assert m.x_d3_source == "auto"
