"""-m gpu: the layout packs' one kernel template (pack.hip: 1-D grid, channel group fastest), bit for bit, in every format.

magnet_pack_split's planes against convnet.split_bf16 through tests/conv_fwd_ref.py's check_planes_exact, as tests/test_gpu_conv_fwd.py
checks the pack kernels, at the shapes where the block index is decoded differently: a pixel tile with a tail, exactly one tile, many
channel groups over less than one tile (the D-Net's skip packs), a ragged last channel group, and a batch-strided input.  Every element
the call does not own (border rows, the other channels) still holds the sentinel the planes were filled with.

The other formats share that decode, and their own tests never reach a wide launch with several channel groups, so each runs at the
same shapes where its entry point accepts them, against the restatement its own test uses: magnet_pack_f16 against the numpy fp16
saturation (tests/test_conv_precision_host.py),
magnet_pack_features against permute + .to(bfloat16) (ctot = C, c_off = 0, dense input, pad 0 and 1; the border of pad 1 is zero).
Their destinations lie between guard bands of the sentinel."""
import numpy as np
import pytest
import torch

from tests import conv_fwd_ref as C
from tests.test_conv_precision_host import assert_f16_bits_equal, f16_sat_bits

pytestmark = pytest.mark.gpu

SENT = -7.0                                        # exact in bf16; no split of N(0, 1) data writes it into both planes


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _sent(shape, dtype, dev):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


PACK = [
    # id                       N  C     h  w   ctot  c_off strided
    ("tile-and-tail-hw132",    2, 256,  6, 22, 320,  64,   False),   # 132 pixels: crosses the 128-pixel tile, 4-pixel tail
    ("one-tile-hw128",         2, 64,   8, 16, 64,   0,    False),
    ("dnet-2048ch-hw60",       1, 2048, 3, 20, 2048, 0,    False),   # less than one tile, 32 channel groups
    ("ragged-C72",             3, 72,   4, 34, 128,  8,    False),   # C not a multiple of 64
    ("batch-strided-input",    2, 256,  6, 22, 320,  64,   True),    # x[:2] of a larger tensor: in_img_stride
]


def _source(gpu, N, Cn, h, w, strided):
    """The fp32 NCHW source of a PACK row on the GPU: dense, or x[:N, :Cn] of a tensor with one more image and 8 more channels."""
    full = torch.randn((N + 1 if strided else N, Cn + 8 if strided else Cn, h, w), generator=_g(11 + Cn + h * w)).to(gpu)
    x = full[:N, :Cn] if strided else full
    if strided:
        assert not x.is_contiguous() and x.stride(0) == (Cn + 8) * h * w
    return x


def _assert_guards(name, buf, fill):
    g = torch.full((C.GUARD,), fill, dtype=buf.dtype, device=buf.device)
    assert torch.equal(buf[:C.GUARD], g) and torch.equal(buf[-C.GUARD:], g), f"{name}: write outside the buffer"


@pytest.mark.parametrize("N,Cn,h,w,ctot,c_off,strided", [p[1:] for p in PACK], ids=[p[0] for p in PACK])
def test_pack_split_row_dense(hip_lib, gpu, request, N, Cn, h, w, ctot, c_off, strided):
    from magnet_amd import lib
    from magnet_amd.convnet import split_bf16
    name = request.node.callspec.id
    x = _source(gpu, N, Cn, h, w, strided)
    hi, lo = (_sent((N, h + 2, w + 2, ctot), torch.bfloat16, gpu) for _ in range(2))
    lib.pack_split(x, hi, lo, ctot, c_off)
    torch.cuda.synchronize()
    eh, el = split_bf16(x.permute(0, 2, 3, 1).contiguous())
    exp = [_sent((N, h + 2, w + 2, ctot), torch.bfloat16, gpu) for _ in range(2)]
    for e, pl in zip(exp, (eh, el)):
        e[:, 1:-1, 1:-1, c_off:c_off + Cn] = pl
    C.check_planes_exact(name, hi, lo, exp[0], exp[1])                 # interior rows, border rows and the other channels


@pytest.mark.parametrize("N,Cn,h,w,ctot,c_off,strided", [p[1:] for p in PACK], ids=[p[0] for p in PACK])
def test_pack_f16_row_dense(hip_lib, gpu, request, N, Cn, h, w, ctot, c_off, strided):
    from magnet_amd import lib
    name = request.node.callspec.id
    x = _source(gpu, N, Cn, h, w, strided)
    buf, body = C.guarded((N, h + 2, w + 2, ctot), gpu, torch.float16, SENT)
    lib.pack_f16(x, body, ctot, c_off)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)
    exp = bits(torch.full((N, h + 2, w + 2, ctot), SENT, dtype=torch.float16))
    exp[:, 1:-1, 1:-1, c_off:c_off + Cn] = f16_sat_bits(x.permute(0, 2, 3, 1).cpu().numpy())      # Cn % 8 == 0: no round-up lanes
    assert_f16_bits_equal(name, bits(body), exp)                       # interior rows, border rows and the other channels
    _assert_guards(name, buf, SENT)


FEATURES = [p for p in PACK if not p[7]]                              # ctot = C, c_off = 0, dense input: the strided row drops out


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Cn,h,w", [p[1:5] for p in FEATURES], ids=[p[0] for p in FEATURES])
def test_pack_features_row_dense(hip_lib, gpu, request, N, Cn, h, w, dtype, pad):
    from magnet_amd import lib
    name = request.node.callspec.id
    x = _source(gpu, N, Cn, h, w, False)
    dt = lib.feat_torch_dtype(lib.feat_enum(dtype))
    buf, body = C.guarded((N, h + 2 * pad, w + 2 * pad, Cn), gpu, dt, SENT)
    got = lib.pack_features(x, lib.feat_enum(dtype), pad=pad, out=body)
    torch.cuda.synchronize()
    exp = torch.nn.functional.pad(x, (pad, pad, pad, pad)).permute(0, 2, 3, 1).contiguous().to(dt)  # RNE for bf16; pad 1: a zero border
    assert got.dtype == exp.dtype and torch.equal(got, exp), f"{name}: {int((got != exp).sum())} elements differ"
    _assert_guards(name, buf, SENT)
