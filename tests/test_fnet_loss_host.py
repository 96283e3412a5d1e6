"""FnetLoss without a GPU: the fp64 restatement of tests/fnet_loss_ref.py equals torch's float64 autograd of the driver's expression
(train_FNet.py:88-104), its bounds hold for an fp32 emulation of the kernel's online form, and the host side (argument checks, the C
ABI's error codes, the defaults of the public interface) behaves as documented.  Nothing is launched here."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from magnet_amd import homography, lib
from magnet_amd.losses import FnetLoss
from magnet_amd.magnet import MAGNET_F
from tests import fnet_loss_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "magnet_hip.h")
MIN_D, MAX_D = 1e-3, 10.0


def _case(B, D, h, w, std, seed, gt_hw=None):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, D, h, w, generator=g, dtype=torch.float64) * std).float()
    H, W = gt_hw or (h, w)
    gt = torch.rand(B, 1, H, W, generator=g) * 12.0                        # some above max_depth
    gt[torch.rand(B, 1, H, W, generator=g) < 0.2] = 0.0                     # missing measurements
    return x, R.sid_centres(D, MIN_D, MAX_D), gt


@pytest.mark.parametrize("shape,std,gt_hw", [((2, 80, 4, 6), 8.0, (10, 14)), ((2, 80, 4, 6), 1.0, None), ((1, 3, 5, 7), 1.0, None),
                                             ((3, 1, 2, 3), 1.0, None), ((1, 256, 2, 3), 30.0, (8, 12))])
def test_restatement_equals_float64_autograd_of_the_driver(shape, std, gt_hw):
    x, d, gt = _case(*shape, std, seed=sum(shape), gt_hw=gt_hw)
    x64 = x.double().requires_grad_(True)
    loss, pred = R.driver_loss_torch(x64, d.double(), gt.double(), MIN_D, MAX_D)
    (loss * 3.0).backward()
    # the restatement takes gt at the volume's resolution, unclipped: clipping commutes with nearest sampling
    gt_lo = torch.nn.functional.interpolate(gt, size=list(shape[2:]), mode="nearest")[:, 0]
    ref = R.fnet_loss_ref(x, d, gt_lo, MIN_D, MAX_D, grad_loss=3.0)
    assert ref["count"] == int(((gt_lo > MIN_D) & (gt_lo <= MAX_D)).sum()) and 0 < ref["count"] < gt_lo.numel()
    np.testing.assert_allclose(ref["pred"].numpy(), pred.detach()[:, 0].numpy(), rtol=1e-13, atol=0)
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-13 * abs(float(loss.detach()))
    scale = float(x64.grad.abs().max())
    # two float64 evaluations: p (d - pred) against autograd's p (w - sum p w); they differ by float64 roundings of terms of size `scale`
    np.testing.assert_allclose(ref["grad"].numpy(), x64.grad.numpy(), rtol=1e-11, atol=1e-12 * scale)


@pytest.mark.parametrize("D,std", [(80, 1.0), (80, 8.0), (256, 30.0), (3, 1.0), (1, 1.0), (24, 8.0)])
@pytest.mark.parametrize("chunk", [R.CHUNK, 1])
def test_bounds_hold_for_the_fp32_online_form(D, std, chunk):
    x, d, gt = _case(2, D, 13, 17, std, seed=D + int(std))
    ref = R.fnet_loss_ref(x, d, gt[:, 0], MIN_D, MAX_D, chunk=chunk)
    pred, m, rz = R.online_fp32(x.numpy(), d.numpy(), chunk=chunk)
    assert np.array_equal(m, x.numpy().max(axis=1))
    worst = R.worst_ratio(torch.from_numpy(pred), ref["pred"], ref["bound_pred"])
    rel = float(((torch.from_numpy(pred).double() - ref["pred"]).abs() / ref["pred"].abs()).max()) / R.U
    print(f"D={D} std={std} chunk={chunk}: worst |err| / bound {worst:.3f}, worst relative error {rel:.1f} u, K = {R.k_const(D, chunk)}")
    assert worst <= 1.0
    # the backward's arithmetic on top of it
    p32, gt32 = pred, gt[:, 0].numpy()
    valid = ref["valid"].numpy()
    c = np.float32(1.0 / ref["count"])
    g = np.where(valid, np.sign(p32 - gt32), 0).astype(np.float32) * c
    t = (g * rz).astype(np.float32)
    e = np.exp((x.numpy() - m[:, None]).astype(np.float32)).astype(np.float32)
    grad = ((t[:, None] * e).astype(np.float32) * (d.numpy()[None, :, None, None] - p32[:, None]).astype(np.float32)).astype(np.float32)
    assert R.worst_ratio(torch.from_numpy(grad), ref["grad"], ref["bound_grad"]) <= 1.0
    if D == 1:
        assert np.array_equal(pred, np.full_like(pred, d.numpy()[0])) and not grad.any()


def test_bound_constants():
    assert R.k_const(80) == 80 + 5 * 5 + 4 and R.k_const(256) == 256 + 5 * 16 + 4 and R.k_const(3) == 3 + 15 + 4
    assert R.rescales(24) == 1 + 8 and R.rescales(80, 1) == 80


def _args(**kw):
    a = dict(loss_fn="l1", min_depth=MIN_D, max_depth=MAX_D); a.update(kw)
    return SimpleNamespace(**a)


def test_fnet_loss_rejects_bad_arguments():
    x, d, gt = torch.zeros(2, 8, 4, 6), torch.zeros(1, 8, 1, 1), torch.zeros(2, 1, 16, 24)
    with pytest.raises(lib.MagnetError, match="GPU tensor"):
        FnetLoss(_args())(x, d, gt)
    with pytest.raises(lib.MagnetError, match="loss_fn 'gaussian'"):
        FnetLoss(_args(loss_fn="gaussian"))(x, d, gt)
    with pytest.raises(lib.MagnetError, match="expected"):
        FnetLoss(_args())(x, d, gt[:1])                                     # another batch
    with pytest.raises(lib.MagnetError, match="expected"):
        FnetLoss(_args())(x, d, gt[:, 0])                                   # (B, H, W)
    with pytest.raises(lib.MagnetError, match="bins"):
        FnetLoss(_args())(x, d[:, :7], gt)
    with pytest.raises(lib.MagnetError, match="D <= 256"):
        FnetLoss(_args())(torch.zeros(1, 257, 2, 2), torch.zeros(257), torch.zeros(1, 1, 2, 2))
    with pytest.raises(lib.MagnetError, match="min_depth"):
        FnetLoss(_args(min_depth=-1.0))(x, d, gt)
    with pytest.raises(lib.MagnetError, match="torch.Tensor"):
        FnetLoss(_args())(x, [1.0] * 8, gt)
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        homography.expected_depth_F(x, d)
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        lib.fnet_loss_forward(x, d.reshape(-1))
    with pytest.raises(lib.MagnetError, match="torch.Tensor"):
        homography.expected_depth_F(x, [1.0] * 8)


def test_new_symbols_are_declared_and_exported(hip_lib):
    text = open(HEADER).read()
    for name in ("magnet_fnet_loss_forward", "magnet_fnet_loss_backward"):
        assert name in lib.API_SYMBOLS and hasattr(hip_lib, name)
        assert re.search(r"MAGNET_API int %s\(const MagnetFnetLossArgs \*args, void \*stream\);" % name, text)
    assert re.search(r"#define MAGNET_HIP_VERSION 500\b", text)              # the header's literal is the library's
    assert re.search(r"typedef struct MagnetFnetLossArgs \{", text)


def test_entry_points_return_codes(hip_lib):
    L = hip_lib
    fwd, bwd = L.magnet_fnet_loss_forward, L.magnet_fnet_loss_backward
    assert fwd(None, None) == lib.E_NULL and bwd(None, None) == lib.E_NULL
    a = lib.MagnetFnetLossArgs()
    assert fwd(ctypes.byref(a), None) == lib.E_NULL and b"NULL" in L.magnet_last_error()
    a.x = a.d = a.pred = 16
    a.B, a.D, a.h, a.w = 1, 0, 4, 4
    assert fwd(ctypes.byref(a), None) == lib.E_DIM                          # D < 1 (gt NULL: the pred-only form needs no more pointers)
    a.D = 257
    assert fwd(ctypes.byref(a), None) == lib.E_DIM and b"D=257" in L.magnet_last_error()
    a.D = 80; a.h = 0
    assert fwd(ctypes.byref(a), None) == lib.E_DIM
    a.h = 4; a.B = -1
    assert fwd(ctypes.byref(a), None) == lib.E_DIM
    a.B = 1; a.min_depth = -0.5
    assert fwd(ctypes.byref(a), None) == lib.E_DIM and b"min_depth" in L.magnet_last_error()
    a.min_depth = float("nan")
    assert fwd(ctypes.byref(a), None) == lib.E_DIM
    a.min_depth = 0.0; a.gt = 16                                            # with gt the loss outputs are required
    assert fwd(ctypes.byref(a), None) == lib.E_NULL
    a.m = a.rz = a.sums = a.loss = 16
    assert fwd(ctypes.byref(a), None) == lib.E_NULL                         # work
    a.work = 16
    assert bwd(ctypes.byref(a), None) == lib.E_NULL                         # grad_loss, grad_x
    a.grad_loss = a.grad_x = 16; a.w = 0
    assert bwd(ctypes.byref(a), None) == lib.E_DIM
    a.w = 4; a.D = 300
    assert bwd(ctypes.byref(a), None) == lib.E_DIM
    a.D = 80; a.min_depth = -1e-3
    assert bwd(ctypes.byref(a), None) == lib.E_DIM
    a.min_depth = 0.0; a.gt = None
    assert bwd(ctypes.byref(a), None) == lib.E_NULL                         # the backward has no gt-less form


def test_public_defaults_keep_the_softmax():
    assert inspect.signature(homography.est_costvolume_F).parameters["softmax"].default is True
    assert inspect.signature(MAGNET_F.forward).parameters["softmax"].default is True
    assert list(inspect.signature(homography.est_costvolume_F).parameters)[:9] == [
        "d_center", "ref_feat", "nghbr_feat", "R", "t", "is_valid", "cam_intrins", "path", "bwd_path"]
    assert list(inspect.signature(MAGNET_F.forward).parameters)[:7] == [
        "self", "ref_img", "nghbr_imgs", "nghbr_poses", "is_valid", "cam_intrins", "d_center"]


def test_d_center_copy_is_cached_by_pointer_and_version():
    d = R.sid_centres(80).view(1, 80, 1, 1)
    a = homography.d_center_device(d, "cpu")
    assert homography.d_center_device(d, "cpu") is a and a.shape == (80,) and a.data_ptr() != d.data_ptr()
    d.mul_(2.0)                                                             # an in-place edit bumps _version: a fresh copy
    b = homography.d_center_device(d, "cpu")
    assert b is not a and torch.equal(b, d.reshape(-1))
    # an entry belongs to the tensor object: another tensor under the same key (a freed tensor's address reused) does not hit
    key = next(k for k, v in homography._D_CENTER_CACHE.items() if v[1] is b)
    other = torch.zeros(80)
    homography._D_CENTER_CACHE[key] = (homography.weakref.ref(other), b)
    c = homography.d_center_device(d, "cpu")
    assert c is not b and torch.equal(c, d.reshape(-1))


def test_worst_ratio_does_not_let_nan_pass():
    ref, bound = torch.ones(3, dtype=torch.float64), torch.full((3,), 0.5, dtype=torch.float64)
    assert R.worst_ratio(torch.tensor([1.0, float("nan"), 1.0]), ref, bound) == float("inf")
    assert R.worst_ratio(torch.tensor([1.0, 1.25, 1.0]), ref, bound) == 0.5
    assert R.worst_ratio(torch.ones(3), ref, torch.zeros(3, dtype=torch.float64)) == 0.0
