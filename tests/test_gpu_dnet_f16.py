"""-m gpu: the D-Net decoder's fp16 single-plane mode (DNetMFMA(precision="fp16"), DNET(precision=...), MAGNET(dnet_precision=...)).

Shape of the runner tests: the seeded decoder on the stand-in encoder with 3 images of 96 x 160, so the decoder's grids are 3 x 5,
6 x 10, 12 x 20 and 24 x 40 (bordered: 105, 288, 924 and 3 276 rows: one ragged tile up to 26 tiles).

Launch audit: lib.conv_mfma is wrapped, and every decoder convolution launch of a run is held to the derived bound of
tests/test_gpu_conv_f16d.py, gamma(taps * cin + 5) (|x| conv |w| + |bias|) + one rounding of the output format, against the fp64
convolution of exactly the planes and weights that launch received.  With split-K the bound is the same: the order of the S - 1
additions is inside gamma (K + 5 roundings bound any summation order of the K products).

Accuracy: tests/dnet_f16_ref.py restates the decoder in float64 with the mode's roundings.  e_fmt is its distance from the plain
float64 decoder, e_hip the HIP mode's: max |diff| / max |ref| for x_feat, mu and sigma.  The bar e_hip <= 2 e_fmt comes from the
format, not from the kernel; e_hip > 10 x the default mode's distance is the negative control (the mode really ran).
Measured on MI355X (profiles/dnet_precision/NOTES.md): x_feat e_fmt 7.66e-4 / e_hip 7.15e-4 / default 1.34e-5, mu 3.86e-4 / 3.93e-4 /
1.12e-5, sigma 4.75e-4 / 4.61e-4 / 9.19e-6; the audit's worst |error| / bound 0.160 unsplit, 0.158 forced, 0.168 under "auto"; final
depth of the end-to-end workload against the default mode 1.6e-4 abs_rel at both refinements (printed, not asserted: the mode is
outside the project's 1e-4 final-depth contract, as INTEGRATION.md says).
"""
import copy

import pytest
import torch

from magnet_amd import fnet, lib
from magnet_amd.dnet import SPLIT_LAYERS, DNetMFMA, gaussian_activation
from magnet_amd.magnet import MAGNET
from magnet_amd.sequence import SequenceRunner
from magnet_amd.standin import make_args, make_dnet, seeded_magnet_weights
from tests import conv_fwd_ref as C
from tests.dnet_f16_ref import decoder_f16_ref
from tests.stubs import procedural_images, seeded_fnet_state
from tests.test_gpu_conv_f16p import _f16_bound
from tests.test_gpu_sequence import CALLS, IMG, T, PerImage, _all_same, _run_calls, _sequence

pytestmark = pytest.mark.gpu

N, H, W = 3, 96, 160
F16D, F16D_SK = "magnet_conv_mfma_f16d", "magnet_conv_mfma_f16d_splitk"
_S = {}


def _setup(gpu):
    """The seeded D-Net on the GPU and the stand-in features of the three images, computed once and never modified."""
    if not _S:
        d = make_dnet().to(gpu)
        with torch.no_grad():
            feats = d.d_net.encoder(procedural_images(N, H, W).to(gpu))
        assert [tuple(feats[i].shape[2:]) for i in (11, 8, 6, 5)] == [(3, 5), (6, 10), (12, 20), (24, 40)]
        _S.update(d=d, dec=d.d_net.decoder, feats=feats)
    return _S["dec"], _S["feats"]


def _audit(monkeypatch, runner, feats, standalone=False):
    """Run once with lib.conv_mfma wrapped; every f16='wide' launch is checked against fp64.  Returns (worst ratio, routes of all calls)."""
    real = lib.conv_mfma
    worst, routes = [0.0], []

    def wrapped(in_hi, in_lo, in_ld, cin, w_hi, w_lo, bias, taps, wp, relu, rows, **kw):
        n = real(in_hi, in_lo, in_ld, cin, w_hi, w_lo, bias, taps, wp, relu, rows, **kw)
        routes.append((kw.get("f16", False), kw.get("tail") is not None, kw.get("split_k")))
        if kw.get("f16") != "wide":
            return n
        torch.cuda.synchronize()
        assert in_lo is None and w_lo is None and in_hi.dtype == torch.float16 and w_hi.dtype == torch.float16 and not relu
        cout, K = w_hi.shape[1], taps * cin
        x = in_hi[:rows, :cin].double()
        conv, b0 = C.conv_ref(x, w_hi.double(), taps, wp, rows, 1)
        mag = b0 / (1.01 * C.LOLO + 1.02 * C.gamma_l(3 * K + 2))
        b = bias.double()[:cout]
        ref, bound = conv + b, C.gamma_l(K + 5) * (mag + b.abs())
        if kw.get("leaky") is not None:
            ref = torch.where(ref < 0, ref * C.f32(kw["leaky"]), ref)
        hp, pad = kw["border"]
        n_img = rows // (hp * wp)
        repad = kw.get("repad", 0)
        if kw.get("out_f32") is not None:
            got = kw["out_f32"].reshape(-1, cout)
        elif kw.get("out_lo") is not None:
            bound = bound + 2.0 ** -16 * (ref.abs() + bound)
            got = kw["out_hi"][:, :cout].double() + kw["out_lo"][:, :cout].double()
        else:
            bound = _f16_bound(ref, bound)
            got = kw["out_hi"][:, :cout]
        ref, bound, written = C.border_and_repad(ref, bound, n_img, hp, wp, pad, repad)
        assert bool(written.all())
        worst[0] = max(worst[0], C.check(f"taps {taps} cin {cin} cout {cout} rows {rows}", got[:ref.shape[0]], ref, bound))
        return n
    monkeypatch.setattr(lib, "conv_mfma", wrapped)
    out = runner.run_standalone(feats) if standalone else runner.run(feats)
    monkeypatch.setattr(lib, "conv_mfma", real)
    return worst[0], routes, out


DECODER = ["conv2", "up1.0", "up1.1", "up2.0", "up2.1", "up3.0", "up3.1"]


@pytest.mark.parametrize("split_k", [0, {"up1.0": 2, "up2.0": 2}, "auto"], ids=["unsplit", "forced", "auto"])
def test_every_decoder_launch_against_fp64_and_the_routes(hip_lib, gpu, monkeypatch, split_k):
    dec, feats = _setup(gpu)
    runner = DNetMFMA(dec, split_k=split_k, precision="fp16")
    worst, routes, _ = _audit(monkeypatch, runner, feats)
    print(f"[dnet fp16 audit, split_k={split_k!r}] worst |error| / bound over the decoder's launches: {worst:.4f}")
    log = runner.launch_log
    S = dict((n, s) for n, _, s in runner.factors_used)
    # run() without x_d3_out: the seven decoder layers, up3.1 once into the heads' planes and once more as NCHW fp32, then the depth head
    assert [l for l, _ in log] == DECODER + ["depth_head", "up3.1"]
    for layer, entry in log:
        if layer in SPLIT_LAYERS:
            assert entry == (F16D_SK if S[layer] > 1 else F16D), (layer, entry)
        else:
            assert entry in ("magnet_conv_mfma", "magnet_conv_mfma_ex"), (layer, entry)          # the head: the bf16x3 fused-tail launch
    wide = [r for r in routes if r[0] == "wide"]
    assert len(wide) == 8 and all(not tail for _, tail, _ in wide)
    heads = [r for r in routes if r[0] != "wide"]
    assert len(heads) == 1 and heads[0][0] is False and heads[0][1]                              # bf16x3 planes with the fused tail
    if split_k == 0:
        assert all(s == 1 for s in S.values())
    elif isinstance(split_k, dict):
        assert {n for n, s in S.items() if s > 1} == {"up1.0", "up2.0"}
    else:
        assert any(s > 1 for s in S.values())                                                    # three small images: "auto" splits
    # the stand-alone form: both heads on today's route
    worst, routes, out = _audit(monkeypatch, runner, feats, standalone=True)
    assert [l for l, _ in runner.launch_log] == DECODER + ["depth_head", "mask_head"]
    assert all(e in ("magnet_conv_mfma", "magnet_conv_mfma_ex") for l, e in runner.launch_log if l.endswith("_head"))
    assert tuple(out.shape) == (N, 2, 4 * 24, 4 * 40) and bool(torch.isfinite(out).all()) and bool((out[:, 1] > 0).all())


def test_default_precision_takes_todays_path_bit_for_bit(hip_lib, gpu):
    dec, feats = _setup(gpu)
    a, b = DNetMFMA(dec), DNetMFMA(dec, precision="bf16x3")
    ga, fa = a(feats)
    gb, fb = b(feats)
    assert torch.equal(ga, gb) and torch.equal(fa, fb)
    assert all(e in ("magnet_conv_mfma", "magnet_conv_mfma_ex") for _, e in a.launch_log) and a.launch_log == b.launch_log
    g16, f16 = DNetMFMA(dec, precision="fp16")(feats)
    assert not torch.equal(f16, fa)                                                              # the mode really is another path


@pytest.mark.parametrize("split_k", [0, {"up1.0": 2, "up2.0": 2, "up3.1": 2}], ids=["unsplit", "forced"])
def test_structure_and_invariance(hip_lib, gpu, split_k):
    dec, feats = _setup(gpu)
    runner = DNetMFMA(dec, split_k=split_k, precision="fp16")
    g1, f1 = runner(feats)
    g2, f2 = runner(feats)
    assert torch.equal(g1, g2) and torch.equal(f1, f2)                                           # two runs are bit-identical
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(f1).all())
    alone = [None if f is None else f[1:2].clone() for f in feats]
    ga, fa = runner(alone)
    assert torch.equal(ga, g1[1:2]) and torch.equal(fa, f1[1:2])                                 # image 1 alone: the bits it has in the batch
    # in place: x_feat of reference frames [0, B) into channels [c_off, c_off + 256) of a sentinel-filled G-Net-style buffer
    B, h, w, ctot, c_off = 2, 24, 40, 384, 64
    ghi = torch.full((B * (h + 2) * (w + 2), ctot), 3.0, dtype=torch.bfloat16, device=gpu); glo = torch.full_like(ghi, 3.0)
    ref_gmms, nghbr_gmms = runner.run(feats, n_ref=B, x_d3_out=(ghi, glo, ctot, c_off))
    assert torch.equal(ref_gmms, g1[:B]) and torch.equal(nghbr_gmms, g1[B:])
    assert [l for l, _ in runner.launch_log] == DECODER + ["up3.1", "depth_head", "depth_head"]
    buf = (ghi.float() + glo.float()).reshape(B, h + 2, w + 2, ctot)
    assert bool((buf[..., :c_off] == 6.0).all()) and bool((buf[..., c_off + 256:] == 6.0).all())
    xs = buf[..., c_off:c_off + 256]
    assert not xs[:, 0].any() and not xs[:, -1].any() and not xs[:, :, 0].any() and not xs[:, :, -1].any()
    torch.testing.assert_close(xs[:, 1:-1, 1:-1].permute(0, 3, 1, 2), f1[:B], rtol=1e-5, atol=1e-5)   # one bf16 split apart
    out = runner.run_standalone(feats)
    assert tuple(out.shape) == (N, 2, 4 * h, 4 * w) and bool(torch.isfinite(out).all()) and bool((out[:, 1] > 0).all())
    assert torch.equal(out, runner.run_standalone(feats))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_accuracy_against_fp64_with_the_formats_own_bar(hip_lib, gpu):
    dec, feats = _setup(gpu)
    with torch.no_grad():
        dec64 = copy.deepcopy(dec).double().eval()
        ref_g, ref_f = gaussian_activation(dec64([None if f is None else f.double() for f in feats]))
        fmt_g, fmt_f = decoder_f16_ref(dec64, feats)
    g16, f16 = DNetMFMA(dec, precision="fp16")(feats)
    g3, f3 = DNetMFMA(dec)(feats)
    rows = []
    for name, ref, fmt, hip, default in (("x_feat", ref_f, fmt_f, f16, f3), ("mu", ref_g[:, 0], fmt_g[:, 0], g16[:, 0], g3[:, 0]),
                                         ("sigma", ref_g[:, 1], fmt_g[:, 1], g16[:, 1], g3[:, 1])):
        rows.append((name, _rel(fmt, ref), _rel(hip, ref), _rel(default, ref), _rel(hip, fmt)))
    for name, e_fmt, e_hip, e_def, e_hf in rows:
        print(f"[dnet fp16 accuracy] {name}: e_fmt {e_fmt:.3e}  e_hip {e_hip:.3e}  default {e_def:.3e}  hip vs restatement {e_hf:.3e}")
    peak = max(float(feats[i].abs().max()) for i in (5, 6, 8, 11))
    print(f"[dnet fp16 accuracy] peak |encoder feature| {peak:.4g}, peak |x_feat| {float(f16.abs().max()):.4g} (fp16 range: 65504)")
    for name, e_fmt, e_hip, e_def, _ in rows:
        assert e_hip <= 2.0 * e_fmt, (name, e_hip, e_fmt)
        assert e_hip > 10.0 * e_def, (name, e_hip, e_def)                                        # negative control: the mode really ran


# ---- MAGNET end to end, on the workload of tests/test_gpu_sequence.py ----------------------------------------------------------------
def _model(gpu, D=5, **kw):
    args = make_args(D=D, iters=2, dpv_h=IMG // 4, dpv_w=IMG // 4, fdim=64, V=2)
    args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
    f = fnet.FNET(args)
    seeded_fnet_state(f.f_net, seed=5)
    f = f.to(gpu).eval()
    d = make_dnet(seed=2, enc_seed=3)
    d.d_net.encoder = PerImage(d.d_net.encoder)
    fkw = dict(f_net=PerImage(f, fnet.FNetMFMA(f.f_net).run)) if kw.get("fnet_precision", "bf16x3") == "bf16x3" else dict(f_net=f)
    model = MAGNET(args, d_net=d, feat_dtype="bf16", dnet_backend="hip", **fkw, **kw).to(gpu).eval()
    seeded_magnet_weights(model, seed=4, gain=0.3)
    return model


def test_magnet_dnet_precision_end_to_end(hip_lib, gpu):
    frames, calls = _sequence(gpu)
    fwd = lambda m: _run_calls(lambda ri, rimg, ni, nimg, *rest: m(rimg, nimg, *rest, mode="test"), frames, calls)
    model = _model(gpu, dnet_precision="fp16")
    assert model._dnet.precision == "fp16"
    got = fwd(model)
    assert all(len(r) == 2 and bool(torch.isfinite(p).all()) for r in got for p in r)
    assert all(e == F16D for l, e in model._dnet.launch_log if l in SPLIT_LAYERS) and len(model._dnet.launch_log) >= 9
    # SequenceRunner.forward equals MAGNET.forward bit for bit under the mode
    seq = _run_calls(SequenceRunner(model, capacity=T).forward, frames, calls)
    assert _all_same(seq, got)
    # against the default mode: printed, not asserted (the mode is outside the 1e-4 contract)
    ref = fwd(_model(gpu))
    for it in range(2):
        abs_rel = max(float(((g[it][:, 0] - r[it][:, 0]).abs() / r[it][:, 0].abs()).mean()) for g, r in zip(got, ref))
        print(f"[magnet dnet_precision fp16 vs bf16x3] refinement {it + 1}: final-depth abs_rel {abs_rel:.3e}")
    assert not _all_same(got, ref)
    # composes with the other two precision modes
    both = _model(gpu, dnet_precision="fp16", conv_precision="fp16", fnet_precision="fp16")
    out = fwd(both)
    assert all(len(r) == 2 and bool(torch.isfinite(p).all()) for r in out for p in r)
    assert both._dnet.precision == "fp16" and both.conv_precision == "fp16" and both.fnet_precision == "fp16"
    assert len(CALLS) == len(out)
