"""-m gpu: DnetLoss on the HIP path (csrc/dnet_loss.hip) against the fp64 restatement and the pointwise bounds of
tests/dnet_loss_ref.py: loss, pred, grad_depth and grad_mask at every shape, for the logit / variance / mask patterns that take each
path, bit-identity with magnet_dnet_upsample_gauss, determinism, strided masks, no host synchronisation, the plain form with its
clamp, and the decoder gradients of a seeded stand-alone D-Net through the fused tail against the torch fp32 tail.

test_end_to_end_decoder_gradients on an MI355X (profiles/dnet_loss/NOTES.md): relative L2 to float64 autograd 2.111e-06 for the torch
fp32 tail and 2.114e-06 for the fused tail; the bar is twice the torch tail's own error, measured in the same test."""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch

from magnet_amd import lib
from magnet_amd.losses import DnetLoss
from magnet_amd.standin import make_dnet
from tests import dnet_loss_ref as R

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 3, 5), (1, 2, 67), (2, 13, 17), (3, 120, 200)]
ARGS = SimpleNamespace(loss_fn="gaussian")


@functools.lru_cache(maxsize=None)
def _case(shape, std):
    """(depth, mask, gt, valid) on the GPU and the fp64 restatement with its bounds, computed once per (shape, std)."""
    t = tuple(x.cuda() for x in R.random_case(*shape, std, seed=100 * shape[1] + shape[2] + int(std)))
    return t + (R.dnet_loss_ref(*t),)


def _run(depth, mask, gt, valid, grad_loss=1.0):
    """Forward and backward through the binding; grad_mask is pre-filled with NaN so that an element the kernel skips shows."""
    loss, sums, pred = lib.dnet_loss_forward(depth, mask, gt, valid)
    gm = torch.full_like(mask, float("nan"))
    gl = torch.tensor(grad_loss, dtype=torch.float32, device=depth.device)
    gd, gm2 = lib.dnet_loss_backward(depth, mask, gt, valid, sums, gl, grad_mask=gm, grad_mask_layout=(0,) + tuple(gm.stride()))
    assert gm2.data_ptr() == gm.data_ptr()
    return loss, sums, pred, gd, gm


def _check(depth, mask, gt, valid, ref, what):
    loss, sums, pred, gd, gm = _run(depth, mask, gt, valid)
    for t, name in ((gd, "grad_depth"), (gm, "grad_mask"), (pred, "pred")):
        assert torch.isfinite(t).all(), f"{what}: {name} holds NaN / inf (an element not written?)"
    assert int(sums[0]) == ref["count"]
    r = dict(pred=R.worst_ratio(pred, ref["pred"], ref["bound_pred"]), grad_depth=R.worst_ratio(gd, ref["grad_depth"], ref["bound_grad_depth"]),
             grad_mask=R.worst_ratio(gm, ref["grad_mask"], ref["bound_grad_mask"]))
    el = abs(float(loss) - ref["loss"])
    print(f"{what}: " + ", ".join(f"{k} {v:.3g} of its bound" for k, v in r.items()) +
          f", loss error {el:.3e} (bound {ref['bound_loss']:.3e}), {ref['count']} valid")
    assert all(v <= 1.0 for v in r.values()), r
    assert el <= ref["bound_loss"]
    return loss, pred, gd, gm


@pytest.mark.parametrize("std", [1.0, 8.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_within_the_bounds_of_the_fp64_restatement(hip_lib, gpu, shape, std):
    depth, mask, gt, valid, ref = _case(shape, std)
    assert 0 < ref["count"] <= gt.numel()
    _check(depth, mask, gt, valid, ref, f"{shape} std {std}")


@pytest.mark.parametrize("pattern", ["equal", "one_tap_1e4", "spread_88", "v_floor", "v_positive", "mu_equals_gt"])
def test_logit_and_variance_patterns(hip_lib, gpu, pattern):
    depth, mask, gt, valid = R.random_case(2, 13, 17, 1.0, seed=len(pattern))
    depth, mask, gt = R.pattern_case(pattern, depth, mask, gt)
    depth, mask, gt, valid = (t.cuda() for t in (depth, mask, gt, valid))
    if pattern == "mu_equals_gt":                                           # d = 0 exactly, everywhere: gt is the kernel's own mu
        gt = lib.dnet_loss_forward(depth, mask, gt, valid)[2][:, 0].contiguous()
    _, pred, gd, gm = _check(depth, mask, gt, valid, R.dnet_loss_ref(depth, mask, gt, valid), pattern)
    if pattern == "v_floor":                                                # away from the border (zero neighbours pull vu up) var is at its floor
        assert (pred[:, 1] >= 1e-10).all() and (pred[:, 1, 4:-4, 4:-4] < 1e-7).all()
    if pattern == "v_positive":
        assert (pred[:, 1, 4:-4, 4:-4] > 1.0).all()
    if pattern == "mu_equals_gt":
        assert torch.equal(pred[:, 0], gt)


@pytest.mark.parametrize("which", ["none", "corner", "border"])
def test_mask_cases(hip_lib, gpu, which):
    depth, mask, gt, _, _ = _case((2, 13, 17), 1.0)
    valid = torch.zeros_like(gt, dtype=torch.bool)
    if which == "corner":
        valid[1, -1, -1] = True
    elif which == "border":
        valid[:, 0], valid[:, -1], valid[:, :, 0], valid[:, :, -1] = True, True, True, True
    ref = R.dnet_loss_ref(depth, mask, gt, valid)
    if which == "none":                                                     # NaN loss (0 / 0), every gradient zero
        loss, sums, _, gd, gm = _run(depth, mask, gt, valid)
        assert torch.isnan(loss) and float(sums[0]) == 0.0
        assert not gd.any() and not gm.any() and not torch.isnan(gd).any() and not torch.isnan(gm).any()
        return
    _, _, gd, gm = _check(depth, mask, gt, valid, ref, which)
    if which == "corner":                                                   # one fine pixel: its coarse pixel's logits of that sub-pixel, its 3x3 depths
        assert ref["count"] == 1
        nz = gm.reshape(2, 9, 4, 4, 13, 17).abs().sum(1)
        assert nz[1, 3, 3, 12, 16] > 0 and int((nz != 0).sum()) == 1
        assert not gd[0].any() and int((gd[1, 0] != 0).sum()) == 4          # the corner's neighbourhood inside the image is 2 x 2


@pytest.mark.parametrize("shape,std", [((2, 13, 17), 8.0), ((1, 2, 67), 1.0), ((3, 120, 200), 1.0)])
def test_pred_is_bit_identical_to_dnet_upsample_gauss(hip_lib, gpu, shape, std):
    depth, mask, gt, valid, _ = _case(shape, std)
    B, h, w = shape
    _, _, pred = lib.dnet_loss_forward(depth, mask, gt, valid)
    head = torch.zeros(B, h + 2, w + 2, 2, device=gpu)                      # the wrapper's padded channel-last layout
    head[:, 1:-1, 1:-1] = depth.permute(0, 2, 3, 1)
    mpad = torch.zeros(B, h + 2, w + 2, 144, device=gpu)
    mpad[:, 1:-1, 1:-1] = mask.permute(0, 2, 3, 1)
    out = torch.empty(B, 2, 4 * h, 4 * w, device=gpu)
    lib.dnet_upsample_gauss(head.reshape(-1, 2), 2, mpad.reshape(-1, 144), 144, B, h, w, out)
    assert torch.equal(out, pred)
    loss2, _, none = lib.dnet_loss_forward(depth, mask, gt, valid, pred=False)   # pred is optional and does not change the loss
    assert none is None and torch.equal(loss2, lib.dnet_loss_forward(depth, mask, gt, valid)[0])


def test_runs_are_bit_identical_and_grad_output_scales_exactly(hip_lib, gpu):
    depth, mask, gt, valid, _ = _case((3, 120, 200), 1.0)
    a, b, c = _run(depth, mask, gt, valid), _run(depth, mask, gt, valid), _run(depth, mask, gt, valid, grad_loss=4.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(c[3], a[3] * 4.0) and torch.equal(c[4], a[4] * 4.0) and torch.equal(c[0], a[0])
    assert a[3].abs().max() > 0 and a[4].abs().max() > 0


def test_strided_masks_give_identical_results(hip_lib, gpu):
    depth, mask, gt, valid, _ = _case((2, 13, 17), 8.0)
    B, h, w = 2, 13, 17
    loss, sums, pred, gd, gm = _run(depth, mask, gt, valid)
    gl = torch.ones((), device=gpu)
    # the same logits held channel-last: a permuted view passes as it is, and the gradient comes back in the same strides
    mcl = mask.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not mcl.is_contiguous() and mcl.stride(1) == 1
    loss2, sums2, pred2 = lib.dnet_loss_forward(depth, mcl, gt, valid)
    gd2, gm2 = lib.dnet_loss_backward(depth, mcl, gt, valid, sums2, gl)
    assert gm2.stride() == mcl.stride()
    assert torch.equal(loss2, loss) and torch.equal(pred2, pred) and torch.equal(gd2, gd) and torch.equal(gm2, gm)
    # and inside a zero-bordered channel-last plane of pitch 160 (the convolution kernel's output layout), addressed by a layout tuple
    ld = 160
    plane = torch.full((B, h + 2, w + 2, ld), float("nan"), device=gpu)
    plane[:, 1:-1, 1:-1, :144] = mask.permute(0, 2, 3, 1)
    gplane = torch.full_like(plane, float("nan"))
    layout = ((w + 2 + 1) * ld, (h + 2) * (w + 2) * ld, 1, (w + 2) * ld, ld)
    loss3, sums3, pred3 = lib.dnet_loss_forward(depth, plane, gt, valid, mask_layout=layout)
    gd3, _ = lib.dnet_loss_backward(depth, plane, gt, valid, sums3, gl, mask_layout=layout, grad_mask=gplane, grad_mask_layout=layout)
    assert torch.equal(loss3, loss) and torch.equal(pred3, pred) and torch.equal(gd3, gd)
    assert torch.equal(gplane[:, 1:-1, 1:-1, :144].permute(0, 3, 1, 2), gm)
    gplane[:, 1:-1, 1:-1, :144] = float("nan")
    assert torch.isnan(gplane).all()                                       # nothing but the 144 channels of the interior was written


def test_forward_and_backward_do_not_synchronise(hip_lib, gpu):
    depth, mask, gt, valid, ref = _case((2, 13, 17), 1.0)
    d, m = depth.clone().requires_grad_(True), mask.clone().requires_grad_(True)
    gt4, valid4 = gt.unsqueeze(1), valid.unsqueeze(1)
    crit = DnetLoss(ARGS)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit((d, m), gt4, valid4)
        (loss * 2.0).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(crit.pred.shape) == (2, 2, 52, 68) and not crit.pred.requires_grad
    assert abs(float(loss.detach()) - ref["loss"]) <= ref["bound_loss"]
    ref2 = R.dnet_loss_ref(depth, mask, gt, valid, grad_loss=2.0)
    assert R.worst_ratio(d.grad, ref2["grad_depth"], ref2["bound_grad_depth"]) <= 1.0
    assert R.worst_ratio(m.grad, ref2["grad_mask"], ref2["bound_grad_mask"]) <= 1.0
    # inputs that are not fp32 are brought to fp32, and the gradient flows back through the cast
    mh = mask.half().requires_grad_(True)
    DnetLoss(ARGS)((depth, mh), gt4, valid4).backward()
    refh = R.dnet_loss_ref(depth, mh.detach().float(), gt, valid)
    assert mh.grad.dtype == torch.float16 and torch.isfinite(mh.grad).all()
    assert R.worst_ratio(mh.grad, refh["grad_mask"], refh["bound_grad_mask"] + refh["grad_mask"].abs() * 2.0 ** -11 + 2.0 ** -24) <= 1.0


@pytest.mark.parametrize("shape", [(2, 6, 9), (3, 130, 210)])
def test_plain_form_against_the_restatement(hip_lib, gpu, shape):
    pred, gt, valid, ns = (t.cuda() if isinstance(t, torch.Tensor) else t for t in R.plain_case(*shape))
    ref = R.dnet_nll_ref(pred, gt, valid, grad_loss=0.5)
    assert int((ref["clamped"] & valid).sum()) == 5 and int(ref["clamped"].sum()) == 6
    loss, sums = lib.dnet_nll_forward(pred, gt, valid)
    grad = lib.dnet_nll_backward(pred, gt, valid, sums, torch.tensor(0.5, device=gpu))
    rg = R.worst_ratio(grad, ref["grad"], ref["bound_grad"])
    el = abs(float(loss) - ref["loss"])
    print(f"plain {shape}: grad {rg:.3g} of its bound, loss error {el:.3e} (bound {ref['bound_loss']:.3e}), {ref['count']} valid")
    assert int(sums[0]) == ref["count"] and el <= ref["bound_loss"] and rg <= 1.0
    assert not grad[:, 1][ref["clamped"]].any()                             # var < 1e-10 and var <= 0: no var gradient
    assert grad[:, 0][ref["clamped"] & valid].abs().min() > 0               # mu keeps its gradient there
    assert not grad.permute(1, 0, 2, 3)[:, ~valid].any()
    # the module, the reference's call: out = pred (B,2,H,W)
    p = pred.clone().requires_grad_(True)
    crit = DnetLoss(ARGS)
    l2 = crit(p, gt.unsqueeze(1), valid.unsqueeze(1))
    (l2 * 0.5).backward()
    assert torch.equal(l2.detach(), loss) and torch.equal(p.grad, grad) and crit.pred is None
    nothing = torch.zeros_like(valid)
    l3, s3 = lib.dnet_nll_forward(pred, gt, nothing)
    assert torch.isnan(l3) and not lib.dnet_nll_backward(pred, gt, nothing, s3, torch.ones((), device=gpu)).any()


def test_end_to_end_decoder_gradients(hip_lib, gpu):
    """A seeded DNET(dnet=True) with the stand-in encoder at 64 x 96 in .train(): the decoder-parameter gradients through the fused loss
    and through the torch fp32 tail, both behind the same fp32 forward, against float64 autograd (on the CPU).  The fused path's
    relative L2 error may exceed the torch fp32 tail's own by at most a factor of 2 (the other summation order)."""
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 64, 96, generator=g)
    gt = torch.rand(2, 1, 64, 96, generator=g) * 3.0 + 1.0
    valid = torch.rand(2, 1, 64, 96, generator=g) < 0.5
    model = make_dnet(dnet=True).train()
    m64 = copy.deepcopy(model).double()
    params64 = list(m64.d_net.decoder.parameters())
    loss64, _ = R.torch_tail(*m64(img.double(), upsample=False), gt.double(), valid)
    ref = torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss64, params64)])

    model = model.to(gpu)
    params = list(model.d_net.decoder.parameters())
    depth, up_mask = model(img.to(gpu), upsample=False)
    gt_g, valid_g = gt.to(gpu), valid.to(gpu)
    loss_t, _ = R.torch_tail(depth, up_mask, gt_g, valid_g)
    crit = DnetLoss(ARGS)
    loss_f = crit((depth, up_mask), gt_g, valid_g)
    g_t = torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss_t, params, retain_graph=True)]).cpu()
    g_f = torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss_f, params)]).cpu()
    e_t, e_f = R.rel_l2(g_t, ref), R.rel_l2(g_f, ref)
    print(f"decoder gradients, relative L2 to float64 autograd: torch fp32 tail {e_t:.3e}, fused tail {e_f:.3e}; "
          f"loss float64 {float(loss64.detach()):.8f}, torch fp32 {float(loss_t.detach()):.8f}, fused {float(loss_f.detach()):.8f}")
    assert float(ref.norm()) > 0 and torch.isfinite(g_f).all()
    assert e_f <= 2.0 * e_t
    assert tuple(crit.pred.shape) == (2, 2, 64, 96)
