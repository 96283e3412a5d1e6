"""The D-Net decoder's host side (magnet_amd/dnet.py): the torch restatement against the reference's own Decoder (golden vectors
from tests/golden/make_golden_dnet.py), the fp64 BatchNorm fold, MAGNET's dnet_backend validation and the ABI mirror of
magnet_conv_mfma_ex.  No GPU needed."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

from magnet_amd import lib
from magnet_amd.dnet import DNET, DenseDepthDecoder, load_seeded_decoder, seeded_decoder_state
from magnet_amd.magnet import MAGNET
from magnet_amd.planes import fold_bn
from magnet_amd.standin import StandinEncoder, StubFNet, make_args, make_dnet, make_dnet_args

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "include", "magnet_hip.h")


@pytest.fixture(scope="module")
def golden_dnet():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_dnet.npz"))


def _features(g, case):
    flist = [None] * 12
    for i in (5, 6, 8, 11):
        flist[i] = torch.from_numpy(g[f"{case}_f{i}"]).double()
    return flist


def test_state_dict_keys_and_shapes_match_the_reference(golden_dnet):
    sd = DenseDepthDecoder().state_dict()
    assert list(sd.keys()) == list(golden_dnet["keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(golden_dnet["shapes"])
    # under DNET: d_net.encoder.* / d_net.decoder.*
    keys = DNET(make_dnet_args(), StandinEncoder()).state_dict().keys()
    assert {k for k in keys if k.startswith("d_net.decoder.")} == {"d_net.decoder." + k for k in sd}
    assert any(k.startswith("d_net.encoder.") for k in keys)


@pytest.mark.parametrize("case", ["A", "B"])
def test_decoder_matches_the_reference_outputs(golden_dnet, case):
    dec = load_seeded_decoder(DenseDepthDecoder()).double().eval()
    d = DNET(make_dnet_args(), nn.Identity())
    d.d_net.decoder = dec
    with torch.no_grad():
        gmm, feat = d.eval()(_features(golden_dnet, case))
    for got, key in ((gmm, "gmm"), (feat, "feat")):
        ref = torch.from_numpy(golden_dnet[f"{case}_{key}"]).double()
        assert got.shape == ref.shape
        rel = float((got - ref).abs().max() / ref.abs().max())
        assert rel < 1e-6, (case, key, rel)


def test_seeded_recipe_is_deterministic_and_order_free():
    shapes = {k: tuple(v.shape) for k, v in DenseDepthDecoder().state_dict().items()}
    a = seeded_decoder_state(shapes, seed=3)
    b = seeded_decoder_state(dict(reversed(list(shapes.items()))), seed=3)
    assert all(np.array_equal(a[k], b[k]) for k in shapes)
    assert not np.array_equal(a["conv2.weight"], seeded_decoder_state(shapes, seed=4)["conv2.weight"])
    assert a["up1._net.4.running_var"].min() >= 0.5


def test_bn_fold_equals_eval_batchnorm_in_fp64():
    dec = load_seeded_decoder(DenseDepthDecoder()).double().eval()
    x = torch.randn(2, 552, 5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    net = dec.up3._net
    with torch.no_grad():
        ref = net[1](net[0](x))
        w, b = fold_bn(net[0], net[1])
        got = nn.functional.conv2d(x, w, b, padding=1)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12


def test_standin_encoder_shapes():
    f = StandinEncoder()(torch.zeros(1, 3, 352, 1216))
    assert [tuple(f[i].shape[1:]) for i in (4, 5, 6, 8, 11)] == [(24, 176, 608), (40, 88, 304), (64, 44, 152), (176, 22, 76), (2048, 11, 38)]
    f = StandinEncoder()(torch.zeros(1, 3, 66, 150))                    # odd sizes round up at every stride-2 stage
    assert [tuple(f[i].shape[2:]) for i in (4, 5, 6, 8, 11)] == [(33, 75), (17, 38), (9, 19), (5, 10), (3, 5)]


def _magnet(d_net, **kw):
    return MAGNET(make_args(), d_net=d_net, f_net=StubFNet(), **kw)


def test_dnet_backend_default_and_validation():
    d = make_dnet()
    assert _magnet(d).dnet_backend == "torch"
    m = _magnet(d, dnet_backend="hip")
    assert m.dnet_backend == "hip" and m._dnet is not None
    assert not any("eye" in k for k in m.state_dict())                 # the runner adds no parameters
    with pytest.raises(lib.MagnetError, match="dnet_backend must be"):
        _magnet(d, dnet_backend="miopen")
    with pytest.raises(lib.MagnetError, match="conv_backend='mfma'"):
        _magnet(d, dnet_backend="hip", conv_backend="torch")
    args = make_args(); args.downsample_ratio = 8
    with pytest.raises(lib.MagnetError, match="downsample_ratio 4"):
        MAGNET(args, d_net=d, f_net=StubFNet(), dnet_backend="hip")
    from magnet_amd.standin import StubDNet
    with pytest.raises(lib.MagnetError, match=r"\.d_net\.encoder and \.d_net\.decoder"):
        _magnet(StubDNet(), dnet_backend="hip")


def test_dnet_backend_rejects_a_groupnorm_decoder():
    d = make_dnet()
    for name in ("up1", "up2", "up3"):
        net = getattr(d.d_net.decoder, name)._net
        net[1] = nn.GroupNorm(8, net[1].num_features)
        net[4] = nn.GroupNorm(8, net[4].num_features)
    with pytest.raises(lib.MagnetError, match="BatchNorm decoder"):
        _magnet(d, dnet_backend="hip")


def test_conv_ex_struct_layout_matches_c(hip_lib):
    A = lib.MagnetConvExArgs
    fields = [f[0] for f in A._fields_]
    prog = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(MagnetConvExArgs));' % HEADER
    for f in fields:
        prog += 'printf(" %%zu", offsetof(MagnetConvExArgs, %s));' % f
    prog += 'printf(" %d %d", MAGNET_ACT_BASE, MAGNET_ACT_LEAKY_RELU);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert vals[0] == ctypes.sizeof(A)
    assert vals[1:1 + len(fields)] == [getattr(A, f).offset for f in fields]
    assert vals[-2:] == [lib.ACT_BASE, lib.ACT_LEAKY_RELU]


def test_conv_ex_and_gauss_head_argument_errors(hip_lib):
    L = hip_lib
    assert L.magnet_conv_mfma_ex(None, None) == 1
    x = lib.MagnetConvExArgs()
    c = x.base
    c.in_hi = c.in_lo = c.w_hi = c.w_lo = c.bias = c.out_hi = c.out_lo = 16
    c.rows, c.cin, c.cout_pad, c.taps, c.wp = 128, 64, 128, 9, 10
    x.act = 7
    assert L.magnet_conv_mfma_ex(ctypes.byref(x), None) == 2 and b"act" in L.magnet_last_error()
    x.act, x.act_slope, c.relu = lib.ACT_LEAKY_RELU, 0.01, 1
    assert L.magnet_conv_mfma_ex(ctypes.byref(x), None) == 2 and b"LeakyReLU" in L.magnet_last_error()
    c.relu, x.act_slope = 0, float("nan")
    assert L.magnet_conv_mfma_ex(ctypes.byref(x), None) == 2 and b"finite" in L.magnet_last_error()
    x.act_slope, c.cin = 0.01, 48
    assert L.magnet_conv_mfma_ex(ctypes.byref(x), None) == 2                       # the base checks apply (cin % 32)
    assert L.magnet_dnet_gauss_head(None, 16, 1, 4, 4, 1, 16, None) == 1
    assert L.magnet_dnet_gauss_head(16, 3, 1, 4, 4, 1, 16, None) == 2               # in_ld even
    assert L.magnet_dnet_gauss_head(20, 16, 1, 4, 4, 1, 16, None) == 4              # in 8-byte aligned
