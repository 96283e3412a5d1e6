"""-m gpu: DNetMFMA(split_k=...) — the decoder's plain layers as split-K launches.  Forced factors against the committed fixtures of
the reference's own Decoder (the tiny grids would never trigger "auto"), batch- and role-independence of forced factors, "auto" on one
480 x 640 image against the fp64 decoder, and split_k=0 bit-identical to the default runner.  The bar is the project's 2e-4 of the
largest magnitude: only the fp32 summation order changes."""
import copy
import os

import numpy as np
import pytest
import torch

from magnet_amd.dnet import SPLIT_LAYERS, DenseDepthDecoder, DNetMFMA, gaussian_activation, load_seeded_decoder, split_factor
from magnet_amd.standin import make_dnet
from tests.stubs import procedural_images

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAR = 2e-4


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _golden_feats(gd, case, gpu):
    feats = [None] * 12
    for i in (5, 6, 8, 11):
        feats[i] = torch.from_numpy(gd[f"{case}_f{i}"]).to(gpu)
    return feats


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("case", ["A", "B"])
def test_forced_factors_match_the_reference_decoder(hip_lib, gpu, case, S):
    gd = np.load(os.path.join(REPO, "tests", "golden", "golden_dnet.npz"))
    forced = {name: S for name in SPLIT_LAYERS}
    feats = _golden_feats(gd, case, gpu)
    runner = DNetMFMA(load_seeded_decoder(DenseDepthDecoder()).to(gpu).eval(), split_k=forced)
    gmm, feat = runner(feats)
    assert [n for n, _, _ in runner.factors_used] == list(SPLIT_LAYERS) + ["up3.1"] and all(s == S for _, _, s in runner.factors_used)
    ref_g, ref_f = torch.from_numpy(gd[f"{case}_gmm"]), torch.from_numpy(gd[f"{case}_feat"])
    errs = dict(x_feat=_rel(feat.cpu(), ref_f), mu=_rel(gmm[:, 0].cpu(), ref_g[:, 0]), sigma=_rel(gmm[:, 1].cpu(), ref_g[:, 1]))
    print(f"DNetMFMA split_k {S} vs reference Decoder, case {case}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < BAR for v in errs.values()), errs
    # the stand-alone form against its own fixture
    ref = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "golden_dnet_standalone.npz"))[f"{case}_out"])
    got = DNetMFMA(load_seeded_decoder(DenseDepthDecoder(dnet=True)).to(gpu).eval(), split_k=forced).run_standalone(feats).cpu()
    errs = dict(mu=_rel(got[:, 0], ref[:, 0]), variance=_rel(got[:, 1], ref[:, 1]))
    print(f"run_standalone split_k {S} vs reference Decoder(dnet=True), case {case}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= BAR for v in errs.values()), errs


def test_forced_factors_are_batch_and_role_independent(hip_lib, gpu):
    d = make_dnet().to(gpu)
    forced = {"conv2": 4, "up1.0": 3, "up1.1": 2, "up2.0": 3, "up2.1": 2, "up3.0": 2, "up3.1": 2}
    runner = DNetMFMA(d.d_net.decoder, split_k=forced)
    with torch.no_grad():
        feats = d.d_net.encoder(procedural_images(3, 256, 320).to(gpu))
    g1, f1 = runner(feats)
    g2, f2 = runner(feats)
    assert torch.equal(g1, g2) and torch.equal(f1, f2)                  # deterministic
    alone = [None if f is None else f[1:2].clone() for f in feats]
    ga, fa = runner(alone)
    assert torch.equal(ga, g1[1:2]) and torch.equal(fa, f1[1:2])        # image 1 of 3 alone: the same bits
    # the in-place x_d3_out form: the same Gaussians, and x_feat of the reference image as the planes of the NCHW form's fp32 values
    h, w = feats[5].shape[2:]
    ghi = torch.zeros(((h + 2) * (w + 2), 320), dtype=torch.bfloat16, device=gpu); glo = torch.zeros_like(ghi)
    r, s = runner.run(feats, n_ref=1, x_d3_out=(ghi, glo, 320, 64))
    assert torch.equal(r, g1[:1]) and torch.equal(s, g1[1:])
    from magnet_amd.planes import split_bf16
    eh, el = split_bf16(f1[:1].permute(0, 2, 3, 1).contiguous())
    buf_h = ghi.reshape(1, h + 2, w + 2, 320)[:, 1:-1, 1:-1, 64:].contiguous()
    buf_l = glo.reshape(1, h + 2, w + 2, 320)[:, 1:-1, 1:-1, 64:].contiguous()
    assert torch.equal(buf_h.view(torch.int16), eh.view(torch.int16)) and torch.equal(buf_l.view(torch.int16), el.view(torch.int16))
    # and not what the unsplit runner computes, bit for bit: the mode was taken
    g0, f0 = DNetMFMA(d.d_net.decoder)(feats)
    assert not torch.equal(f0, f1)
    assert _rel(f1, f0) < 1e-5


def test_auto_on_one_image(hip_lib, gpu):
    d = make_dnet().to(gpu)
    with torch.no_grad():
        feats = d.d_net.encoder(procedural_images(1, 480, 640).to(gpu))
        dec64 = copy.deepcopy(d.d_net.decoder).double().eval()
        ref_g, ref_f = gaussian_activation(dec64([None if f is None else f.double() for f in feats]))
    runner = DNetMFMA(d.d_net.decoder, split_k="auto")
    gmm, feat = runner(feats)
    errs = dict(x_feat=_rel(feat, ref_f), mu=_rel(gmm[:, 0], ref_g[:, 0]), sigma=_rel(gmm[:, 1], ref_g[:, 1]))
    print("DNetMFMA split_k auto vs fp64 at 480 x 640 (N = 1): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < BAR for v in errs.values()), errs
    # the record of the factors used is the rule's
    chunks = dict(zip(SPLIT_LAYERS, (64, 70, 32, 34, 16, 18, 8)))
    n_tiles = dict(zip(SPLIT_LAYERS, (16, 8, 8, 4, 4, 2, 2)))
    used = runner.factors_used
    assert [n for n, _, _ in used] == list(SPLIT_LAYERS) + ["up3.1"]    # run(): up3.1 for the planes and again for the NCHW x_feat
    for name, rows, S in used:
        assert S == split_factor((rows + 127) // 128, n_tiles[name], chunks[name]), (name, rows, S)
    assert any(S > 1 for _, _, S in used)
    g0, f0 = DNetMFMA(d.d_net.decoder)(feats)
    print("factors: " + ", ".join(f"{n} {S}" for n, _, S in used) + f"; x_feat vs split_k=0: {_rel(feat, f0):.2e}")
    assert not (torch.equal(g0, gmm) and torch.equal(f0, feat))         # the mode was taken


def test_split_k_zero_is_the_default_path(hip_lib, gpu):
    d = make_dnet().to(gpu)
    with torch.no_grad():
        feats = d.d_net.encoder(procedural_images(2, 256, 320).to(gpu))
    a, b = DNetMFMA(d.d_net.decoder), DNetMFMA(d.d_net.decoder, split_k=0)
    (ga, fa), (gb, fb) = a(feats), b(feats)
    assert torch.equal(ga, gb) and torch.equal(fa, fb)
    assert all(S == 1 for _, _, S in b.factors_used) and "splitk.work" not in b._bufs
    ds = make_dnet(dnet=True).to(gpu)
    assert torch.equal(DNetMFMA(ds.d_net.decoder).run_standalone(feats), DNetMFMA(ds.d_net.decoder, split_k=0).run_standalone(feats))
