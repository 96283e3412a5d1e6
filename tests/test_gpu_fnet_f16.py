"""-m gpu: the F-Net on the single-plane fp16 format (FNetMFMA(precision="fp16"), MAGNET(fnet_precision="fp16")).

The four non-GEMM kernels (`magnet_*_f16`) at the shapes of tests/test_gpu_fnet.py, against fp64 with derived bounds; then the whole
runner: equalities that must hold bit for bit, the default path untouched, and the accuracy of the mode, measured against the same
module's torch fp32 forward (never against the default HIP path) and recorded in the docstrings below.

Bounds of the small kernels: tests/elementwise_fwd_ref.py (stem_ref, avgpool_ref, bilinear_ref with fmt="f16"; derived in its
docstring); space to depth is a move: bit-exact.  tests/test_gpu_elementwise_fwd.py runs the same restatements at the edge shapes, in
both plane formats.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from magnet_amd import fnet, lib
from magnet_amd.planes import to_f16_sat
from tests.conv_fwd_ref import check
from tests.elementwise_fwd_ref import avgpool_ref, bilinear_ref, stem_ref
from tests.stubs import StubDNet, make_args, procedural_images, seeded_fnet_state, seeded_magnet_weights

pytestmark = pytest.mark.gpu

FILL = -7.0                                                          # finite sentinel of the fp16 buffers (a border must stay 0, not this)


def _filled(shape, gpu):
    return torch.full(shape, FILL, dtype=torch.float16, device=gpu)


def _only_written(name, got, mask):
    """Everything outside `mask` still holds the sentinel."""
    assert bool((got[~mask] == FILL).all()), f"{name}: an element outside the written region changed"


def test_stem_f16(hip_lib, gpu):
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 37, 50, generator=g); w = torch.randn(32, 3, 3, 3, generator=g) * 0.2; b = torch.randn(32, generator=g)
    H2, W2 = 19, 25
    out = _filled((2, H2 + 2, W2 + 2, 32), gpu)
    lib.fnet_stem_f16(img.to(gpu), w.reshape(32, 27).contiguous().to(gpu), b.to(gpu), out.view(-1, 32))
    ref, bound = stem_ref(img, w.reshape(32, 27), b, "f16")
    got = out.cpu()
    worst = check("stem_f16", got[:, 1:-1, 1:-1], ref, bound)
    m = torch.zeros(got.shape, dtype=torch.bool); m[:, 1:-1, 1:-1] = True
    _only_written("stem_f16", got, m)
    print(f"[stem_f16] worst ratio {worst:.4f}")


def test_space_to_depth_f16(hip_lib, gpu):
    x = to_f16_sat(torch.randn(2, 11, 14, 32, generator=torch.Generator().manual_seed(2)) * 3)     # odd height: phase rows beyond the edge
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    H4, W4 = 6, 7
    out = _filled((2, H4 + 4, W4 + 4, 128), gpu)
    lib.space_to_depth_f16(xp.reshape(-1, 32).to(gpu), out.view(-1, 128), 2, 32, 11, 14, 2)
    got = out.cpu()
    xs = F.pad(x, (0, 0, 0, 0, 0, 1))                                                              # virtual zero row 11
    for py in (0, 1):
        for px in (0, 1):
            ph = py * 2 + px
            assert torch.equal(got[:, 2:-2, 2:-2, ph * 32:(ph + 1) * 32].view(torch.int16), xs[:, py::2, px::2].contiguous().view(torch.int16))
    m = torch.zeros(got.shape, dtype=torch.bool); m[:, 2:-2, 2:-2] = True
    _only_written("space_to_depth_f16", got, m)


@pytest.mark.parametrize("k", [8, 16, 64])
def test_avgpool_f16(hip_lib, gpu, k):
    x = to_f16_sat(torch.randn(2, 64, 80, 128, generator=torch.Generator().manual_seed(3)) * 4)
    buf = to_f16_sat(torch.randn(2, 68, 84, 320, generator=torch.Generator().manual_seed(30)))      # the other channels and the border hold data
    buf[:, 2:-2, 2:-2, 64:192] = x
    ph, pw = 64 // k, 80 // k
    out = _filled((2 * ph * pw + 8, 128), gpu)
    lib.avgpool_cl_f16(buf.reshape(-1, 320).to(gpu)[:, 64:192], 320, 2, 64, 80, 2, k, 128, out)
    ref, bound = avgpool_ref(x, k, "f16")
    got = out.cpu()
    worst = check(f"avgpool_f16 k={k}", got[:2 * ph * pw], ref, bound)
    assert bool((got[2 * ph * pw:] == FILL).all())
    print(f"[avgpool_f16 k={k}] worst ratio {worst:.4f}")


@pytest.mark.parametrize("ph,pw", [(1, 2), (3, 5), (15, 20)])
def test_upsample_bilinear_f16(hip_lib, gpu, ph, pw):
    q = torch.randn(2, ph, pw, 32, generator=torch.Generator().manual_seed(4))
    h, w = 60, 80
    out = _filled((2, h + 4, w + 4, 320), gpu)
    lib.upsample_bilinear_cl_f16(q.reshape(-1, 32).to(gpu), 32, ph, pw, 32, out.view(-1, 320)[:, 224:256], 320, 2, h, w, 2)
    ref, bound = bilinear_ref(q, h, w, "f16")
    got = out.cpu()
    worst = check(f"upsample_f16 {ph}x{pw}", got[:, 2:-2, 2:-2, 224:256], ref, bound)
    # the reference itself against ATen's bilinear (fp32 arithmetic on both sides: the existing test's tolerance)
    exp = F.interpolate(q.permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    np.testing.assert_allclose(ref.float().numpy(), exp.numpy(), rtol=0, atol=2e-5)
    m = torch.zeros(got.shape, dtype=torch.bool); m[:, 2:-2, 2:-2, 224:256] = True
    _only_written("upsample_f16", got, m)
    print(f"[upsample_f16 {ph}x{pw}] worst ratio {worst:.4f}")


# ---- the whole F-Net -----------------------------------------------------------------------------------------------------------
def _psm(seed, gpu):
    return seeded_fnet_state(fnet.PSMNet(feature_dim=64), seed=seed).eval().to(gpu)


def test_f16_equalities_bit_for_bit(hip_lib, gpu):
    """fp16 mode: the two-stream split == one stream (9 images of 256 x 256, n_ref in {2, 5, 9}); one image alone == the same image
    inside that batch; the matcher-layout outputs == the NCHW output re-laid-out; bf16 storage == RNE of the fp32 output."""
    m = _psm(13, gpu)
    run = fnet.FNetMFMA(m, precision="fp16")
    assert run.split_min_images <= 9
    img = procedural_images(9, 256, 256).to(gpu)
    one = fnet.FNetMFMA(m, precision="fp16"); one.split_min_images = 10 ** 9
    nchw = run.run(img)
    assert bool(torch.isfinite(nchw).all()) and torch.equal(nchw, one.run(img))
    for n_ref in (2, 5, 9):
        a32 = [t.clone() for t in run.run(img, n_ref=n_ref, feat_dtype="fp32")]
        b32 = one.run(img, n_ref=n_ref, feat_dtype="fp32")
        assert torch.equal(a32[0], b32[0]) and torch.equal(a32[1], b32[1]), n_ref
        assert torch.equal(a32[0], nchw[:n_ref].permute(0, 2, 3, 1)) and torch.equal(a32[1][:, 1:-1, 1:-1], nchw[n_ref:].permute(0, 2, 3, 1))
        assert a32[1].numel() == 0 or (not a32[1][:, 0].any() and not a32[1][:, :, -1].any())
        ab = run.run(img, n_ref=n_ref, feat_dtype="bf16")
        assert ab[0].dtype == torch.bfloat16 and torch.equal(ab[0], a32[0].to(torch.bfloat16)) and torch.equal(ab[1], a32[1].to(torch.bfloat16))
    for i in (0, 8):
        alone = one.run(img[i:i + 1].contiguous())
        assert torch.equal(alone[0], nchw[i]), f"image {i}"


def test_default_precision_is_untouched(hip_lib, gpu):
    """FNetMFMA(m) and FNetMFMA(m, precision="bf16x3") are the same path: bitwise equal on the same build; and an fp16 runner on the
    same module does not disturb it (separate packs, separate buffers)."""
    m = _psm(3, gpu)
    img = procedural_images(2, 256, 256).to(gpu)
    a = fnet.FNetMFMA(m).run(img)
    f16 = fnet.FNetMFMA(m, precision="fp16").run(img)
    b = fnet.FNetMFMA(m, precision="bf16x3").run(img)
    assert torch.equal(a, b)
    assert not torch.equal(a, f16)                                    # the mode does change the arithmetic


# max |feat_fp16 - feat_torch_fp32| / max |feat|, measured on an MI355X (2 images; seeds 3, 7, 10 of seeded_fnet_state):
#     256 x 320:  1.046e-3  1.256e-3  1.499e-3        258 x 330:  9.79e-4  1.227e-3  1.407e-3        (rms relative error 6.8 - 8.2e-4;
#     the default path on the same inputs: 1.5 - 2.2e-5).  A host emulation that rounds only the convolutions' operands gave 0.8 -
#     1.0e-3: this mode also rounds the residual stream where it is stored, once per residual unit.
ACCURACY_BAR = 3.0e-3                                                # 2 x the worst measured value (1.499e-3)


@pytest.mark.parametrize("seed", [3, 7, 10])
@pytest.mark.parametrize("hw", [(256, 320), (258, 330)])
def test_f16_accuracy_vs_torch_fp32(hip_lib, gpu, hw, seed):
    """max |d| / max |feat| of the fp16 mode against the same module's torch fp32 forward, 2 images.
    Measured 0.98e-3 .. 1.50e-3 (the six values stand above ACCURACY_BAR and in profiles/fnet_precision/NOTES.md); the bar is 2 x the
    worst of the six, because the rounding noise moves with the seed.  A value above 4e-3 would be a bug, not a bar."""
    H, W = hw
    m = _psm(seed, gpu)
    img = procedural_images(2, H, W).to(gpu)
    with torch.no_grad():
        ref = m(img)
    out = fnet.FNetMFMA(m, precision="fp16").run(img)
    dflt = fnet.FNetMFMA(m).run(img)
    assert out.shape == ref.shape
    scale = ref.abs().max()
    err = ((out - ref).abs().max() / scale).item()
    rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    err0 = ((dflt - ref).abs().max() / scale).item()
    print(f"[fnet fp16 accuracy] {H}x{W} seed {seed}: max err / max|feat| = {err:.3e} (rms rel {rms:.3e}; default path {err0:.3e})")
    assert err < ACCURACY_BAR


G10_BAR = 2.4e-3                                                     # 2 x the measured 1.187e-3


def test_f16_G10_vs_reference_golden(hip_lib, gpu, golden):
    """The metric of test_G10_fnet_mfma_vs_reference_golden, fp16 mode, against the reference's samples.  Measured on an MI355X:
    max err / max |feat| = 1.187e-3 (the default path's bar there is 2e-4); the per-channel mean |feat| moves by at most 5.1e-3
    relative (printed, not asserted: the default path's 1e-3 tolerance on it is a statement about fp32-grade arithmetic)."""
    m = seeded_fnet_state(fnet.PSMNet(feature_dim=64), seed=10).eval()
    img = procedural_images(2, 256, 320)
    out = fnet.FNetMFMA(m.to(gpu), precision="fp16").run(img.to(gpu)).cpu()
    assert tuple(out.shape) == (2, 64, 64, 80)
    scale = float(np.abs(golden["G10_feat_sparse"]).max())
    err = np.abs(out[:, :, ::4, ::4].numpy() - golden["G10_feat_sparse"]).max() / scale
    am = np.abs(out.abs().mean(dim=(0, 2, 3)).numpy() / golden["G10_feat_absmean"] - 1).max()
    print(f"[fnet fp16 G10] max err / max|feat| = {err:.3e}; per-channel |mean| off by at most {am:.2e} (relative)")
    assert err < G10_BAR


E2E_BAR = {"fp32": 8.2e-5, "bf16": 1.35e-4}                          # 2 x the measured 4.056e-5 / 6.707e-5


@pytest.mark.parametrize("feat_dtype", ["fp32", "bf16"])
def test_magnet_fnet_precision_end_to_end(hip_lib, gpu, feat_dtype):
    """The MAGNET of test_magnet_with_fnet_mfma with fnet_precision 'fp16' against 'bf16x3', same inputs, same metric (mean |d mu| / mu
    of the final depth), with fp32 and with bf16 feature storage on both sides.  Measured on an MI355X: 4.06e-5 with fp32 features,
    6.71e-5 with bf16 features — on this workload (seeded weights) both are inside the project's 1e-4 contract on final depth, the
    second with little room (the default path itself sits at 2e-5 against the torch F-Net)."""
    from magnet_amd.magnet import MAGNET
    from magnet_amd import synth
    args = make_args(D=16, iters=2, dpv_h=64, dpv_w=80, fdim=64, V=2)
    args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
    f = seeded_fnet_state(fnet.FNET(args).f_net, seed=5)
    wl = synth.Workload("t", "scannet", 64, 80, V=2, D=16, F=64)
    inp = synth.make_inputs(wl, B=2, seed=11)
    ref_img = procedural_images(2, 256, 320).to(gpu); nb = procedural_images(4, 256, 320).flip(0).to(gpu)
    outs = {}
    for prec in ("bf16x3", "fp16"):
        fn = fnet.FNET(args); fn.f_net = f
        model = MAGNET(args, d_net=StubDNet(0), f_net=fn, feat_dtype=feat_dtype, fnet_precision=prec).to(gpu).eval()
        seeded_magnet_weights(model, seed=4)
        assert model._fnet_runner().precision == prec
        with torch.no_grad():
            outs[prec] = model(ref_img, nb, inp["nghbr_poses"].to(gpu), inp["is_valid"], inp["cam_intrins"], mode="test")[-1][:, 0].cpu()
    a, b = outs["fp16"], outs["bf16x3"]
    assert bool(torch.isfinite(a).all())
    rel = ((a - b).abs() / b.abs().clamp_min(1e-3)).mean().item()
    print(f"[magnet fnet_precision fp16 vs bf16x3, feat {feat_dtype}] mean |d mu|/mu = {rel:.3e}")
    assert rel < E2E_BAR[feat_dtype]
