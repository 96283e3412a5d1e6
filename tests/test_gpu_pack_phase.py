"""-m gpu: magnet_pack_split's wide kernel (1-D grid, channel group fastest, streaming accesses), bit for bit.

The planes against convnet.split_bf16 through tests/conv_fwd_ref.py's check_planes_exact, as tests/test_gpu_conv_fwd.py checks the
pack kernels, at the shapes where the block index is decoded differently: a pixel tile with a tail, exactly one tile, many channel
groups over less than one tile (the D-Net's skip packs), a ragged last channel group, and a batch-strided input.  Every element the
call does not own (border rows, the other channels) still holds the sentinel the planes were filled with."""
import pytest
import torch

from tests import conv_fwd_ref as C

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


@pytest.mark.parametrize("N,Cn,h,w,ctot,c_off,strided", [p[1:] for p in PACK], ids=[p[0] for p in PACK])
def test_pack_split_row_dense(hip_lib, gpu, request, N, Cn, h, w, ctot, c_off, strided):
    from magnet_amd import lib
    from magnet_amd.convnet import split_bf16
    name = request.node.callspec.id
    full = torch.randn((N + 1 if strided else N, Cn + 8 if strided else Cn, h, w), generator=_g(11 + Cn + h * w)).to(gpu)
    x = full[:N, :Cn] if strided else full
    if strided:
        assert not x.is_contiguous() and x.stride(0) == (Cn + 8) * h * w
    hi, lo = (_sent((N, h + 2, w + 2, ctot), torch.bfloat16, gpu) for _ in range(2))
    lib.pack_split(x, hi, lo, ctot, c_off)
    torch.cuda.synchronize()
    eh, el = split_bf16(x.permute(0, 2, 3, 1).contiguous())
    exp = [_sent((N, h + 2, w + 2, ctot), torch.bfloat16, gpu) for _ in range(2)]
    for e, pl in zip(exp, (eh, el)):
        e[:, 1:-1, 1:-1, c_off:c_off + Cn] = pl
    C.check_planes_exact(name, hi, lo, exp[0], exp[1])                 # interior rows, border rows and the other channels
