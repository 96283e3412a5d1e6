"""The stand-alone D-Net's host side (DNET(dnet=True), magnet_amd/dnet.py): the torch restatement against the reference's own
Decoder(dnet=True) + activation_G (golden vectors from tests/golden/make_golden_dnet_standalone.py), DNET's backend argument, the ABI
growth by magnet_dnet_upsample_gauss, its wrapper's argument checks, and the fp64 restatement of the kernel
(tests/dnet_standalone_ref.py) against the reference formulas, with two planted defects it must tell apart.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from magnet_amd import lib
from magnet_amd.dnet import DNET, DenseDepthDecoder, DNetMFMA, check_decoder, gaussian_activation, load_seeded_decoder, upsample_depth_via_mask
from magnet_amd.standin import StandinEncoder, make_dnet, make_dnet_args
from tests.dnet_standalone_ref import pad_cl, upsample_gauss_ref

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "include", "magnet_hip.h")


@pytest.mark.parametrize("case", ["A", "B"])
def test_torch_standalone_dnet_matches_the_reference_outputs(case):
    g = np.load(os.path.join(REPO, "tests", "golden", "golden_dnet.npz"))
    ref = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "golden_dnet_standalone.npz"))[f"{case}_out"]).double()
    flist = [None] * 12
    for i in (5, 6, 8, 11):
        flist[i] = torch.from_numpy(g[f"{case}_f{i}"]).double()
    d = DNET(make_dnet_args(), nn.Identity(), dnet=True)
    d.d_net.decoder = load_seeded_decoder(DenseDepthDecoder(dnet=True)).double().eval()
    with torch.no_grad():
        got = d.eval()(flist)
    assert got.shape == ref.shape == (flist[5].shape[0], 2, 4 * flist[5].shape[2], 4 * flist[5].shape[3])
    for c, name in ((0, "mu"), (1, "variance")):
        rel = float((got[:, c] - ref[:, c]).abs().max() / ref[:, c].abs().max())
        assert rel < 1e-6, (case, name, rel)                                   # the fixture is stored as float32


def test_dnet_backend_argument():
    for dn in (False, True):
        d = DNET(make_dnet_args(), StandinEncoder(), dnet=dn)
        assert d.backend == "torch" and d._runner is None                      # the default is unchanged
        h = DNET(make_dnet_args(), StandinEncoder(), dnet=dn, backend="hip")
        assert h.backend == "hip" and isinstance(h._runner, DNetMFMA)
        assert list(h.state_dict().keys()) == list(d.state_dict().keys())      # the runner adds no parameters
    assert make_dnet(dnet=True, backend="hip").dnet and not make_dnet().dnet
    with pytest.raises(lib.MagnetError, match="backend must be 'torch' or 'hip'"):
        DNET(make_dnet_args(), StandinEncoder(), dnet=True, backend="miopen")
    with pytest.raises(lib.MagnetError, match="downsample_ratio 8"):
        DNET(make_dnet_args(downsample_ratio=8), StandinEncoder(), dnet=True, backend="hip")
    args = make_dnet_args(); args.output_type = "R"
    with pytest.raises(lib.MagnetError, match="output_type 'R'"):
        DNET(args, StandinEncoder(), dnet=True, backend="hip")
    args = make_dnet_args(); args.DNET_architecture = "DenseDepth_GN"
    with pytest.raises(lib.MagnetError, match="DenseDepth_GN"):
        DNET(args, StandinEncoder(), dnet=True, backend="hip")


def test_hip_backend_rejects_a_groupnorm_decoder_and_a_foreign_mask_head():
    dec = DenseDepthDecoder(dnet=True)
    check_decoder(dec, standalone=True)
    for name in ("up1", "up2", "up3"):
        net = getattr(dec, name)._net
        net[1] = nn.GroupNorm(8, net[1].num_features); net[4] = nn.GroupNorm(8, net[4].num_features)
    with pytest.raises(lib.MagnetError, match="BatchNorm decoder"):
        check_decoder(dec, standalone=True)
    dec = DenseDepthDecoder(dnet=True)
    dec.mask_head[4] = nn.Conv2d(128, 9 * 64, 1)                               # the ratio-8 head
    check_decoder(dec)                                                         # MaGNet's form does not read it
    with pytest.raises(lib.MagnetError, match="mask head"):
        check_decoder(dec, standalone=True)


def test_abi_grows_by_one_symbol(hip_lib):
    assert "magnet_dnet_upsample_gauss" in lib.API_SYMBOLS
    text = open(HEADER).read()
    assert re.search(r"MAGNET_API int magnet_dnet_upsample_gauss\(const float \*head, int32_t head_ld, const float \*mask, int32_t mask_ld,"
                     r"\s*int32_t N,\s*int32_t h, int32_t w, float \*out, void \*stream\);", text)
    assert re.search(r"#define MAGNET_HIP_VERSION 500\b", text)
    assert hasattr(hip_lib, "magnet_dnet_upsample_gauss")
    L = hip_lib
    assert L.magnet_dnet_upsample_gauss(None, 16, 16, 144, 1, 4, 4, 16, None) == 1             # NULL
    assert L.magnet_dnet_upsample_gauss(16, 3, 16, 144, 1, 4, 4, 16, None) == 2                # head_ld even
    assert L.magnet_dnet_upsample_gauss(16, 16, 16, 140, 1, 4, 4, 16, None) == 2               # mask_ld >= 144
    assert L.magnet_dnet_upsample_gauss(16, 16, 16, 146, 1, 4, 4, 16, None) == 2               # mask_ld % 4
    assert L.magnet_dnet_upsample_gauss(16, 16, 16, 144, 1, 0, 4, 16, None) == 2               # h > 0
    assert L.magnet_dnet_upsample_gauss(20, 16, 16, 144, 1, 4, 4, 16, None) == 4               # head 8-byte aligned
    assert L.magnet_dnet_upsample_gauss(16, 16, 24, 144, 1, 4, 4, 16, None) == 4               # mask 16-byte aligned
    assert L.magnet_dnet_upsample_gauss(16, 16, 16, 144, 1, 4, 4, 24, None) == 4               # out 16-byte aligned


def test_wrapper_rejects_bad_shapes_and_pitches():
    N, h, w = 2, 3, 5
    rows = N * (h + 2) * (w + 2)
    head, mask, out = torch.zeros(rows, 16), torch.zeros(rows, 144), torch.zeros(N, 2, 4 * h, 4 * w)
    lib.check_dnet_upsample_gauss(head, 16, mask, 144, N, h, w, out)           # the good call passes the checks
    bad = [
        (dict(head_out=head[:-1]), "head output"), (dict(head_ld=8), "head output"), (dict(head_ld=3, head_out=torch.zeros(rows, 3)), "even"),
        (dict(head_out=torch.zeros(rows, 32)[:, :16]), "head output"),          # a channel view: pitch 32 under a declared 16
        (dict(mask_out=mask[:, :140]), "mask_ld|mask logits"), (dict(mask_ld=160), "mask logits"), (dict(mask_out=mask[:rows - 1]), "mask logits"),
        (dict(mask_out=mask.double()), "float32"), (dict(out=torch.zeros(N, 2, 4 * h, 4 * w + 4)), "out must be"),
        (dict(out=torch.zeros(N, 2, 4 * w, 4 * h).transpose(2, 3)), "out must be"), (dict(N=0), "bad dims"), (dict(h=h + 1), "does not hold"),
    ]
    for kw, msg in bad:
        a = dict(head_out=head, head_ld=16, mask_out=mask, mask_ld=144, N=N, h=h, w=w, out=out); a.update(kw)
        with pytest.raises(lib.MagnetError, match=msg):
            lib.check_dnet_upsample_gauss(**a)
    with pytest.raises(lib.MagnetError, match="GPU only"):                      # no CPU fallback
        lib.dnet_upsample_gauss(head, 16, mask, 144, N, h, w, out)


def _random_case(seed, N, h, w, head_ld=16, mask_ld=160):
    rng = np.random.default_rng(seed)
    head = rng.standard_normal((N, 2, h, w)) * 2.0
    logits = rng.standard_normal((N, 144, h, w)) * 3.0
    return head, logits, pad_cl(head, head_ld, fill=7.5), pad_cl(logits, mask_ld, fill=-2.0)


def _reference_formulas(head, logits):
    up = upsample_depth_via_mask(torch.from_numpy(head), torch.from_numpy(logits), 4)      # D_dense_depth.py:85-100
    return gaussian_activation(up, magnet=False).numpy()                                   # DNET.py:55-60


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (3, 1, 6)])
def test_numpy_restatement_equals_the_reference_formulas(shape):
    N, h, w = shape
    head, logits, head_pad, mask_pad = _random_case(11, N, h, w)
    ref = _reference_formulas(head, logits)
    got, bound = upsample_gauss_ref(head_pad, 16, mask_pad, 160, N, h, w, with_bound=True)
    assert got.shape == ref.shape == (N, 2, 4 * h, 4 * w)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-13)
    assert (bound > 0).all() and bound.max() < 1e-4                             # an fp32-sized bound, not a loose one


@pytest.mark.parametrize("defect", ["act_first", "taps_transposed"])
def test_numpy_restatement_rejects_planted_defects(defect):
    N, h, w = 2, 5, 7
    head, logits, head_pad, mask_pad = _random_case(12, N, h, w)
    ref = _reference_formulas(head, logits)
    good, bound = upsample_gauss_ref(head_pad, 16, mask_pad, 160, N, h, w, with_bound=True)
    broken = upsample_gauss_ref(head_pad, 16, mask_pad, 160, N, h, w, defect=defect)
    assert (np.abs(good - ref) <= bound).all()
    over = np.abs(broken - ref) > bound
    assert over[:, 1].mean() > 0.5                                             # far outside the kernel's bound on most of the variance plane
    if defect == "taps_transposed":
        assert over[:, 0].mean() > 0.5                                         # and on mu; 'act_first' leaves mu alone
    else:
        np.testing.assert_allclose(broken[:, 0], ref[:, 0], rtol=1e-13, atol=1e-13)
