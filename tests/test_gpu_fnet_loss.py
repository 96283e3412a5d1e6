"""-m gpu: FnetLoss on the HIP path (csrc/fnet_loss.hip) against the fp64 restatement and the pointwise bounds of
tests/fnet_loss_ref.py: pred, loss and grad_x at every shape and for logit patterns that take each path through the online form, the
masks, determinism, the public interface (expected_depth_F, FnetLoss, MAGNET_F's raw volume) and the eval_fnet.py driver.

The bars of test_end_to_end_against_the_driver_expression are 4 x torch's own relative L2 distance to the fp64 restatement on the same
raw volume (floored at one fp32 ulp for the scalar loss); the test prints every distance.  None has been recorded from an MI355X yet
(profiles/fnet_loss/NOTES.md)."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from magnet_amd import homography, lib, synth
from magnet_amd.losses import FnetLoss
from tests import fnet_loss_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_D, MAX_D = 1e-3, 10.0
SHAPES = [(1, 1, 3, 5), (2, 3, 5, 7), (2, 80, 13, 17), (1, 256, 4, 9), (3, 8, 120, 200), (1, 80, 120, 160)]


def _gt(B, h, w, g):
    """About a fifth missing (0), a sixth above max_depth, the rest valid; a few exactly at the two thresholds."""
    gt = torch.rand(B, h, w, generator=g) * 12.0
    gt[torch.rand(B, h, w, generator=g) < 0.2] = 0.0
    gt.view(-1)[0] = MAX_D                                                 # gt == max_depth is valid (not gt > max_depth)
    gt.view(-1)[1] = MIN_D                                                 # gt == min_depth is not
    return gt


@functools.lru_cache(maxsize=None)
def _case(shape, std):
    """(x, d, gt) on the GPU and the fp64 restatement with its bounds, computed once per (shape, std)."""
    B, D, h, w = shape
    g = torch.Generator().manual_seed(1000 * D + h + int(std))
    x = (torch.randn(B, D, h, w, generator=g) * std).cuda()
    d = R.sid_centres(D, MIN_D, MAX_D).cuda()
    gt = _gt(B, h, w, g).cuda()
    return x, d, gt, R.fnet_loss_ref(x, d, gt, MIN_D, MAX_D)


def _run(x, d, gt, grad_loss=1.0):
    """Forward and backward through the binding; grad_x is pre-filled with NaN so that an element the kernel skips shows."""
    loss, pred, m, rz, sums = lib.fnet_loss_forward(x, d, gt, MIN_D, MAX_D)
    out = torch.full_like(x, float("nan"))
    gl = torch.tensor(grad_loss, dtype=torch.float32, device=x.device)
    grad = lib.fnet_loss_backward(x, d, gt, pred, m, rz, sums, gl, MIN_D, MAX_D, out=out)
    assert grad.data_ptr() == out.data_ptr()
    return loss, pred, sums, grad


def _check(x, d, gt, ref, what):
    loss, pred, sums, grad = _run(x, d, gt)
    assert not torch.isnan(grad).any() and not torch.isinf(grad).any(), f"{what}: grad_x holds NaN / inf (an element not written?)"
    assert torch.isfinite(pred).all()
    assert int(sums[0]) == ref["count"]
    rp = R.worst_ratio(pred, ref["pred"], ref["bound_pred"])
    rg = R.worst_ratio(grad, ref["grad"], ref["bound_grad"])
    el = abs(float(loss) - ref["loss"])
    print(f"{what}: pred {rp:.3f} of its bound, grad {rg:.3f}, loss error {el:.3e} (bound {ref['bound_loss']:.3e}), "
          f"{ref['count']} valid, {ref['marginal']} marginal")
    assert rp <= 1.0 and rg <= 1.0 and el <= ref["bound_loss"]
    return loss, pred, grad


@pytest.mark.parametrize("std", [1.0, 8.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_within_the_bounds_of_the_fp64_restatement(hip_lib, gpu, shape, std):
    x, d, gt, ref = _case(shape, std)
    assert 0 < ref["count"] < gt.numel()
    _, pred, grad = _check(x, d, gt, ref, f"{shape} std {std}")
    if shape[1] == 1:                                                      # one bin: pred is d_0 and the gradient vanishes, exactly
        assert torch.equal(pred, torch.full_like(pred, float(d[0]))) and not grad.any()


def _pattern(name, B, D, h, w):
    g = torch.Generator().manual_seed(D + len(name))
    j = torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)
    pix = torch.rand(B, 1, h, w, generator=g)
    if name == "ascending":                                                # the maximum moves at every step
        return j * (0.25 + pix) + pix
    if name == "descending":                                               # it never moves
        return -j * (0.25 + pix) + pix
    if name == "equal":
        return (pix * 6 - 3).expand(B, D, h, w).contiguous()
    if name == "one_hot_1e4":                                              # one bin at +1e4 (another one per pixel), the rest at 0
        x = torch.zeros(B, D, h, w)
        x.scatter_(1, torch.randint(0, D, (B, 1, h, w), generator=g), 1e4)
        return x
    if name == "spread_88":                                                # overflows without the max subtraction
        x = torch.rand(B, D, h, w, generator=g) * 176 - 88
        x[:, 0], x[:, D - 1] = 88.0, -88.0
        return x
    raise ValueError(name)


@pytest.mark.parametrize("name", ["ascending", "descending", "equal", "one_hot_1e4", "spread_88"])
@pytest.mark.parametrize("shape", [(2, 80, 13, 17), (1, 256, 4, 9), (2, 3, 5, 7)])
def test_logit_patterns(hip_lib, gpu, shape, name):
    B, D, h, w = shape
    x = _pattern(name, *shape).cuda()
    d = R.sid_centres(D, MIN_D, MAX_D).cuda()
    gt = _gt(B, h, w, torch.Generator().manual_seed(5)).cuda()
    _check(x, d, gt, R.fnet_loss_ref(x, d, gt, MIN_D, MAX_D), f"{name} {shape}")


def test_no_valid_pixel(hip_lib, gpu):
    x, d, _, _ = _case((2, 80, 13, 17), 1.0)
    for gt in (torch.zeros(2, 13, 17, device=gpu), torch.full((2, 13, 17), 11.0, device=gpu), torch.full((2, 13, 17), float("nan"), device=gpu)):
        loss, pred, sums, grad = _run(x, d, gt)
        assert torch.isnan(loss) and float(sums[0]) == 0.0 and not grad.any() and not torch.isnan(grad).any()


def test_single_valid_pixel(hip_lib, gpu):
    x, d, _, _ = _case((2, 80, 13, 17), 8.0)
    gt = torch.zeros(2, 13, 17, device=gpu)
    gt[1, 7, 11] = 2.5
    ref = R.fnet_loss_ref(x, d, gt, MIN_D, MAX_D)
    assert ref["count"] == 1
    _, _, grad = _check(x, d, gt, ref, "single valid pixel")
    keep = torch.zeros_like(grad, dtype=torch.bool)
    keep[1, :, 7, 11] = True
    assert not grad[~keep].any() and grad[keep].any()


def test_excluded_pixels_and_count(hip_lib, gpu):
    x, d, _, _ = _case((2, 3, 5, 7), 1.0)
    gt = torch.full((2, 5, 7), 3.0, device=gpu)
    gt[0, 0, :] = MAX_D + 1e-3                                             # above max_depth
    gt[0, 1, :] = MIN_D                                                    # not above min_depth
    gt[0, 2, :] = 0.0
    gt[0, 3, 0] = MAX_D                                                    # still valid
    ref = R.fnet_loss_ref(x, d, gt, MIN_D, MAX_D)
    assert ref["count"] == 70 - 21
    loss, pred, sums, grad = _run(x, d, gt)
    assert float(sums[0]) == 49.0 and not grad[0, :, :3].any() and grad[0, :, 3, 0].any()
    _check(x, d, gt, ref, "excluded pixels")


def test_pred_equal_to_gt_gives_a_zero_gradient(hip_lib, gpu):
    x = torch.randn(1, 1, 3, 5, device=gpu)
    d = torch.tensor([2.75], device=gpu)
    gt = torch.full((1, 3, 5), 2.75, device=gpu)
    loss, pred, sums, grad = _run(x, d, gt)
    assert float(loss) == 0.0 and float(sums[0]) == 15.0 and torch.equal(pred, gt) and not grad.any()
    # and with three bins of the same centre: pred == gt up to rounding or exactly, never a NaN
    x3, d3 = torch.randn(1, 3, 3, 5, device=gpu), torch.full((3,), 2.75, device=gpu)
    _, _, _, grad3 = _run(x3, d3, gt)
    assert torch.isfinite(grad3).all()


def test_bit_identical_and_scaled_exactly_by_the_upstream_gradient(hip_lib, gpu):
    x, d, gt, _ = _case((3, 8, 120, 200), 1.0)
    l1, _, _, g1 = _run(x, d, gt)
    l2, _, _, g2 = _run(x, d, gt)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    # GradScaler's 2^16: c = grad_loss / count scales exactly and so does every product (logits of standard deviation 1: no
    # factor comes near the subnormal range)
    _, _, _, gs = _run(x, d, gt, grad_loss=65536.0)
    assert torch.equal(gs, g1 * 65536.0) and g1.abs().max() > 0


def test_expected_depth_equals_the_loss_forward(hip_lib, gpu):
    for shape in ((2, 80, 13, 17), (2, 3, 5, 7)):
        x, d, gt, ref = _case(shape, 8.0)
        pred = lib.fnet_loss_forward(x, d, gt, MIN_D, MAX_D)[1]
        e = homography.expected_depth_F(x, d.view(1, -1, 1, 1))
        assert e.shape == (shape[0], 1, shape[2], shape[3]) and torch.equal(e[:, 0], pred) and not e.requires_grad
        assert R.worst_ratio(e[:, 0], ref["pred"], ref["bound_pred"]) <= 1.0


def _args():
    return SimpleNamespace(loss_fn="l1", min_depth=MIN_D, max_depth=MAX_D)


def test_module_interpolates_the_ground_truth_as_the_driver(hip_lib, gpu):
    B, D, h, w = 2, 80, 13, 17
    x, d, _, _ = _case((B, D, h, w), 8.0)
    gt_hi = _gt(B, 4 * h, 4 * w, torch.Generator().manual_seed(9)).unsqueeze(1).cuda()
    gt_lo = F.interpolate(gt_hi, size=[h, w], mode="nearest")
    crit = FnetLoss(_args())
    res = []
    for gt in (gt_hi, gt_lo):
        xr = x.clone().requires_grad_(True)
        loss = crit(xr, d.view(1, D, 1, 1), gt)
        loss.backward()
        assert crit.pred_dmap.shape == (B, 1, h, w) and not crit.pred_dmap.requires_grad
        res.append((loss.detach(), xr.grad, crit.pred_dmap))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    ref = R.fnet_loss_ref(x, d, gt_lo[:, 0], MIN_D, MAX_D)                 # and it is the loss of the restatement
    assert abs(float(res[0][0]) - ref["loss"]) <= ref["bound_loss"]
    assert R.worst_ratio(res[0][1], ref["grad"], ref["bound_grad"]) <= 1.0
    # the driver clips before it samples; clipping commutes with nearest sampling
    clipped = gt_hi.clone(); clipped[clipped > MAX_D] = 0.0
    assert torch.equal(crit(x, d, clipped), res[0][0])


def test_no_host_synchronisation(hip_lib, gpu):
    x, d, gt, _ = _case((2, 80, 13, 17), 1.0)
    crit = FnetLoss(_args())
    d4 = d.view(1, -1, 1, 1)
    gt4 = gt.unsqueeze(1)
    crit(x.clone().requires_grad_(True), d4, gt4).backward()               # first call: library load, the cached copy of d_center
    xr = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(xr, d4, gt4)
        (loss * 65536.0).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(xr.grad).all() and xr.grad.any()


def test_sync_debug_mode_catches_a_synchronisation(gpu):
    """Control of the test above: this build of torch implements the mode (boolean indexing, the driver's own tail, trips it)."""
    p, m = torch.ones(8, device=gpu), torch.ones(8, device=gpu) > 0
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            p[m]
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _e2e_inputs(gpu):
    wl = synth.Workload("f", "scannet", 20, 28, V=3, D=32, F=32)           # the shape of test_gpu_costvolume_f::test_softmax_chain_gradient
    inp = synth.make_inputs(wl, B=2, seed=3)
    poses = inp["nghbr_poses"]
    cam = {"intM": inp["cam_intrins"]["intM"], "unit_ray_array_2D": inp["cam_intrins"]["unit_ray_array_2D"]}
    fixed = (poses[:, :, :3, :3].to(gpu), poses[:, :, :3, 3].to(gpu), inp["is_valid"], cam)
    return inp["ref_feat"].to(gpu), inp["nghbr_feat"].to(gpu), fixed


def test_end_to_end_against_the_driver_expression(hip_lib, gpu):
    """est_costvolume_F(softmax=False) + FnetLoss against the default est_costvolume_F + the driver's torch expression.  On the same raw
    volume torch's fp32 tail and the HIP tail are both compared with the fp64 restatement (relative L2): the HIP path may be at most 4
    times as far as torch (other summation order, other exp); for the scalar loss the bar is floored at one fp32 ulp (2 u |loss|), since
    torch's fp32 loss can be the correctly rounded one.  The feature gradients are compared in the same way: the fp64 grad_x, rounded to
    fp32, goes through the same cost-volume backward, and each path's feature gradients may be at most 4 times as far from that as torch's.
    The distances are printed; none is recorded from an MI355X yet (profiles/fnet_loss/NOTES.md)."""
    D, h, w = 32, 20, 28
    rf0, sf0, fixed = _e2e_inputs(gpu)
    dc = R.sid_centres(D, MIN_D, MAX_D).view(1, D, 1, 1).to(gpu)
    gt = _gt(2, 4 * h, 4 * w, torch.Generator().manual_seed(8)).unsqueeze(1).to(gpu)
    gt_clip = gt.clone(); gt_clip[gt_clip > MAX_D] = 0.0

    def leaves():
        return rf0.clone().requires_grad_(True), sf0.clone().requires_grad_(True)

    # the HIP tail
    rf, sf = leaves()
    raw = homography.est_costvolume_F(dc, rf, sf, *fixed, softmax=False)
    raw.retain_grad()
    crit = FnetLoss(_args())
    loss_h = crit(raw, dc, gt)
    loss_h.backward()
    hip = (loss_h.detach(), raw.grad, rf.grad, sf.grad)
    # the driver's tail
    rf, sf = leaves()
    cv = homography.est_costvolume_F(dc, rf, sf, *fixed)
    loss_t, pred_t = R.driver_loss_torch(cv, dc, gt, MIN_D, MAX_D, raw=False)
    loss_t.backward()
    x32 = raw.detach().clone().requires_grad_(True)
    R.driver_loss_torch(x32, dc, gt, MIN_D, MAX_D)[0].backward()
    tor = (loss_t.detach(), x32.grad, rf.grad, sf.grad)
    # fp64 on the same raw volume, and its gradient through the same cost-volume backward
    gt_lo = F.interpolate(gt, size=[h, w], mode="nearest")[:, 0]
    ref = R.fnet_loss_ref(raw.detach(), dc.view(-1), gt_lo, MIN_D, MAX_D)
    rf, sf = leaves()
    homography.est_costvolume_F(dc, rf, sf, *fixed, softmax=False).backward(gradient=ref["grad"].float())
    f64 = (ref["loss"], ref["grad"], rf.grad, sf.grad)
    assert 0 < ref["count"] < gt_lo.numel()
    assert R.worst_ratio(crit.pred_dmap[:, 0], ref["pred"], ref["bound_pred"]) <= 1.0
    el_h, el_t = abs(float(hip[0]) - f64[0]) / f64[0], abs(float(tor[0]) - f64[0]) / f64[0]
    print(f"loss: fp64 {f64[0]:.9f}; relative distance torch {el_t:.3e}, hip {el_h:.3e}")
    assert el_h <= max(4 * el_t, 2 * R.U) and el_h * f64[0] <= ref["bound_loss"]
    for name, i in (("grad_x", 1), ("grad_ref_feat", 2), ("grad_nghbr_feat", 3)):
        r_t, r_h = R.rel_l2(tor[i], f64[i]), R.rel_l2(hip[i], f64[i])
        print(f"{name}: relative L2 distance to fp64: torch {r_t:.3e}, hip {r_h:.3e}, hip to torch {R.rel_l2(hip[i], tor[i]):.3e}")
        assert r_t < 1e-5, "the torch tail itself is off: the comparison means nothing"
        assert r_h <= 4 * r_t, name
    assert R.worst_ratio(hip[1], ref["grad"], ref["bound_grad"]) <= 1.0


def test_eval_fnet_driver(hip_lib, gpu):
    """eval_fnet.py on two synthetic windows in a fresh process: the 12-column metric line with nll 0."""
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "eval_fnet.py"), "--frames", "2"],
                         capture_output=True, text=True, timeout=330)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert "F-Net" in lines[-3] and lines[-2].split() == "abs_rel abs_diff sq_rel rmse rmse_log irmse log_10 silog a1 a2 a3 NLL".split()
    vals = [float(v) for v in lines[-1].split()]
    assert len(vals) == 12 and vals[-1] == 0.0 and all(v == v for v in vals) and vals[1] > 0
