"""-m gpu: the stand-alone D-Net on the HIP path (DNET(dnet=True, backend='hip'), DNetMFMA.run_standalone): the tail kernel
magnet_dnet_upsample_gauss pointwise against its fp64 restatement, run_standalone against the reference's own Decoder(dnet=True)
(golden_dnet_standalone.npz) and against an fp64 torch decoder at the C2 and KITTI shapes, determinism, the DNET backend switch, and
eval_dnet.py's validate() against a host restatement of test_DNet.py's."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from magnet_amd import lib
from magnet_amd.dnet import DenseDepthDecoder, DNetMFMA, gaussian_activation, load_seeded_decoder
from magnet_amd.standin import make_dnet
from tests.dnet_standalone_ref import pad_cl, upsample_gauss_ref, validate_host
from tests.stubs import procedural_images

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAR = 2e-4                       # max|d| / max|ref| on mu and on variance: the bar the dnet=False outputs are held to (test_gpu_dnet.py)


@pytest.mark.parametrize("case", [(1, 1, 1, 2, 144), (2, 5, 7, 16, 160), (3, 9, 37, 16, 144), (2, 1, 6, 4, 148)])
def test_upsample_gauss_kernel_pointwise(hip_lib, gpu, case):
    """The kernel alone against the fp64 restatement, element by element.  The bound is derived from the kernel's arithmetic in
    tests/dnet_standalone_ref.py (upsample_gauss_ref, with_bound=True): per tap the rounding of x - max (|d| U after the exponential),
    a 1-ulp expf (2 U), the 8 additions and the exp errors of the denominator, its reciprocal, the two products and the 8 additions of
    the sum of 9 -- weighted by w[t] |v[t]| -- then for the variance the 1-Lipschitz ELU, a 1-ulp expm1f and the two additions.
    Nothing in it is fitted to a measured error.  Inputs: logits N(0, 3^2) with +-80 planted, v across the ELU knee (negative, exactly
    zero over whole neighbourhoods, positive), border rows of the head full of a value that must not be read, pitches wider than the
    channels used.  Sentinels on both sides of the output show that nothing outside (N, 2, 4h, 4w) is written."""
    N, h, w, head_ld, mask_ld = case
    rng = np.random.default_rng([31, N, h, w])
    head = (rng.standard_normal((N, 2, h, w)) * 2.0).astype(np.float32)
    head[:, 1, :, : (w + 1) // 2] -= 3.0                                        # well below the knee on one side
    if h >= 5:
        head[0, 1, :4, -4:] = 0.0                                              # whole 3x3 neighbourhoods of exact zeros
        head[-1, 1, -3:, -3:] = 40.0
    logits = (rng.standard_normal((N, 144, h, w)) * 3.0).astype(np.float32)
    sel = rng.random(logits.shape)
    logits[sel < 0.02] = 80.0
    logits[sel > 0.98] = -80.0
    head_pad = pad_cl(head, head_ld, fill=np.float32(7.5))                      # border rows and spare channels: never read
    mask_pad = pad_cl(logits, mask_ld, fill=np.float32(-2.0))
    ref, bound = upsample_gauss_ref(head_pad, head_ld, mask_pad, mask_ld, N, h, w, with_bound=True)
    n_out, guard = N * 2 * 16 * h * w, 64
    buf = torch.full((guard + n_out + guard,), -777.0, device=gpu)
    out = buf[guard:guard + n_out].view(N, 2, 4 * h, 4 * w)
    lib.dnet_upsample_gauss(torch.from_numpy(head_pad).to(gpu), head_ld, torch.from_numpy(mask_pad).to(gpu), mask_ld, N, h, w, out)
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    assert (buf[:guard] == -777.0).all() and (buf[guard + n_out:] == -777.0).all()
    assert np.isfinite(got).all() and not (got == -777.0).any()                 # every element written
    err = np.abs(got - ref)
    ratio = float((err / bound).max())
    print(f"dnet_upsample_gauss N={N} {h}x{w} ld {head_ld}/{mask_ld}: max err {err.max():.3e}, max err/bound {ratio:.3f}, "
          f"v range [{ref[:, 1].min():.3e}, {ref[:, 1].max():.3e}]")
    assert (err <= bound).all(), ratio
    assert (got[:, 1] > 0).all()                                                # a variance


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _errs(got, ref):
    return dict(mu=_rel(got[:, 0], ref[:, 0]), variance=_rel(got[:, 1], ref[:, 1]))


@pytest.mark.parametrize("case", ["A", "B"])
def test_run_standalone_matches_the_reference_decoder(hip_lib, gpu, case):
    gd = np.load(os.path.join(REPO, "tests", "golden", "golden_dnet.npz"))
    ref = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "golden_dnet_standalone.npz"))[f"{case}_out"])
    dec = load_seeded_decoder(DenseDepthDecoder(dnet=True)).to(gpu).eval()
    feats = [None] * 12
    for i in (5, 6, 8, 11):
        feats[i] = torch.from_numpy(gd[f"{case}_f{i}"]).to(gpu)
    got = DNetMFMA(dec).run_standalone(feats)
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_contiguous()
    errs = _errs(got.cpu(), ref)
    print(f"run_standalone vs reference Decoder(dnet=True), case {case}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= BAR for v in errs.values()), errs


@pytest.mark.parametrize("shape", [("C2", 2, 480, 640), ("KITTI", 1, 352, 1216)])
def test_run_standalone_against_fp64(hip_lib, gpu, shape):
    name, N, H, W = shape
    d = make_dnet(dnet=True).to(gpu)
    with torch.no_grad():
        feats = d.d_net.encoder(procedural_images(N, H, W).to(gpu))
        dec64 = copy.deepcopy(d.d_net.decoder).double().eval()
        ref = gaussian_activation(dec64([None if f is None else f.double() for f in feats]), magnet=False)
    got = DNetMFMA(d.d_net.decoder).run_standalone(feats)
    assert tuple(got.shape) == (N, 2, H, W)
    errs = _errs(got, ref)
    print(f"run_standalone vs fp64 at {name} (N = {N}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= BAR for v in errs.values()), errs


def test_run_standalone_deterministic_and_batch_independent(hip_lib, gpu):
    d = make_dnet(dnet=True).to(gpu)
    runner = DNetMFMA(d.d_net.decoder)
    with torch.no_grad():
        feats = d.d_net.encoder(procedural_images(3, 256, 320).to(gpu))
    o1 = runner.run_standalone(feats)
    o2 = runner.run_standalone(feats)
    assert o1.data_ptr() != o2.data_ptr() and torch.equal(o1, o2)
    alone = [None if f is None else f[1:2].clone() for f in feats]
    assert torch.equal(runner.run_standalone(alone), o1[1:2])
    # the MaGNet form on the same runner is unchanged by the stand-alone calls around it
    g1, f1 = DNetMFMA(d.d_net.decoder)(feats)
    g2, f2 = runner(feats)
    assert torch.equal(g1, g2) and torch.equal(f1, f2)
    assert torch.equal(runner.run_standalone(feats), o1)
    d.train()
    with pytest.raises(lib.MagnetError, match=r"\.eval\(\)"):
        runner.run_standalone(feats)


def test_dnet_hip_backend_matches_torch(hip_lib, gpu, monkeypatch):
    t = make_dnet(dnet=True, backend="torch").to(gpu)
    m = make_dnet(dnet=True, backend="hip").to(gpu)
    assert all(torch.equal(a, b) for a, b in zip(t.state_dict().values(), m.state_dict().values()))
    img = procedural_images(2, 256, 320).to(gpu)
    with torch.no_grad():
        ref = t(img)
    real = DenseDepthDecoder.forward

    def no_torch_decoder(*a, **k):
        raise AssertionError("the torch decoder ran")
    monkeypatch.setattr(DenseDepthDecoder, "forward", no_torch_decoder)
    with torch.no_grad():
        got = m(img)
    assert got.shape == ref.shape == (2, 2, 256, 320)
    errs = _errs(got, ref)
    print("DNET(dnet=True) backend hip vs torch fp32: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= BAR for v in errs.values()), errs
    # .train(): the torch forward runs and BatchNorm's running statistics move
    monkeypatch.setattr(DenseDepthDecoder, "forward", real)

    def no_hip(*a, **k):
        raise AssertionError("DNetMFMA ran in training mode")
    monkeypatch.setattr(DNetMFMA, "run_standalone", no_hip)
    bn = m.d_net.decoder.up3._net[4]
    before, count = bn.running_mean.clone(), int(bn.num_batches_tracked)
    m.train()
    with torch.no_grad():
        out = m(img)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert int(bn.num_batches_tracked) == count + 1 and not torch.equal(bn.running_mean, before)


def test_dnet_hip_backend_magnet_form_equals_the_runner(hip_lib, gpu):
    m = make_dnet(dnet=False, backend="hip").to(gpu)
    img = procedural_images(2, 256, 320).to(gpu)
    with torch.no_grad():
        gmm, feat = m(img)
        ref_gmm, ref_feat = DNetMFMA(m.d_net.decoder).run(m.d_net.encoder(img))
    assert gmm.shape == (2, 2, 64, 80) and feat.shape == (2, 256, 64, 80)
    assert torch.equal(gmm, ref_gmm) and torch.equal(feat, ref_feat)


@pytest.mark.parametrize("crop", [None, "garg"])
def test_eval_dnet_validate_equals_the_host_restatement(hip_lib, gpu, crop):
    """eval_dnet.validate() on 4 synthetic frames against test_DNet.py:40-71 + utils.compute_depth_errors restated in float64 numpy
    on the same HIP outputs (bit-identical run to run), to 1e-6 relative."""
    sys.path.insert(0, REPO)
    import argparse
    import eval_dnet as E
    model = make_dnet(dnet=True, backend="hip").to(gpu).eval()
    args = argparse.Namespace(min_depth=1e-3, max_depth=10.0, garg_crop=crop == "garg", eigen_crop=False)
    H, W = 96, 128
    got = E.validate(model, args, E.SyntheticFrames(4, 1, H, W, seed=5), gpu)
    outs, gts = [], []
    with torch.no_grad():
        for fr in E.SyntheticFrames(4, 1, H, W, seed=5):
            outs.append(model(fr["img"].to(gpu)).cpu().numpy()); gts.append(fr["depth"].numpy())
    ref = validate_host(outs, gts, 1e-3, 10.0, crop=crop)
    assert set(got) == set(ref) == set(E.M.METRIC_ORDER)
    for k in E.M.METRIC_ORDER:
        print(f"eval_dnet {k}: device {got[k]:.9g} host {ref[k]:.9g}")
    for k in E.M.METRIC_ORDER:
        assert np.isfinite(got[k]) and abs(got[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, got[k], ref[k])


def test_eval_dnet_command_line(hip_lib, gpu, tmp_path):
    log = tmp_path / "test_acc.txt"
    out = subprocess.run([sys.executable, os.path.join(REPO, "eval_dnet.py"), "--frames", "3", "--batch", "2", "--input_height", "96",
                          "--input_width", "128", "--log", str(log)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    text = log.read_text()
    assert "abs_rel" in text and "synthetic frames=3" in text and "nan" not in text.lower() and text.count("\n") == 4


def test_eval_dnet_on_a_scannet_folder(hip_lib, gpu, tmp_path):
    pytest.importorskip("PIL")
    sys.path.insert(0, REPO)
    import argparse
    import eval_dnet as E
    from magnet_amd import data
    from tests.test_data_loader import _make_scene
    _make_scene(str(tmp_path), "scene0001_00", 6, raw_wh=(160, 128))
    ds = data.ScanNetFolder(str(tmp_path), [("scene0001_00", 2), ("scene0001_00", 3), ("scene0001_00", 5)], n_views=2, window_radius=0,
                            input_hw=(96, 128), dpv_hw=(24, 32))
    model = make_dnet(dnet=True, backend="hip").to(gpu).eval()
    m = E.validate(model, argparse.Namespace(min_depth=1e-3, max_depth=10.0), E.FolderFrames(ds, 2), gpu)
    assert set(m) == set(E.M.METRIC_ORDER) and all(np.isfinite(v) for v in m.values())
