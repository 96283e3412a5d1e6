"""DnetLoss without a GPU: the fp64 restatement of tests/dnet_loss_ref.py equals torch's float64 autograd of the torch tail
(dnet.upsample_depth_via_mask + gaussian_activation(magnet=False) + the reference's loss expression), its bounds hold for an fp32
emulation of the kernels' arithmetic and fail for two deliberately wrong gradients, and the host side (the header, the binding, the
argument checks, DNET's upsample=False) behaves as documented.  Nothing is launched here."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from magnet_amd import lib
from magnet_amd.dnet import DNET
from magnet_amd.losses import DnetLoss
from magnet_amd.standin import StandinEncoder, make_dnet, make_dnet_args
from tests import dnet_loss_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "magnet_hip.h")


@pytest.mark.parametrize("shape,std", [((1, 1, 1), 1.0), ((2, 3, 5), 1.0), ((2, 3, 5), 8.0), ((1, 5, 1), 8.0), ((1, 2, 7), 30.0)])
def test_restatement_equals_float64_autograd_of_the_torch_tail(shape, std):
    depth, mask, gt, valid = R.random_case(*shape, std, seed=sum(shape) + int(std))
    d64, m64 = depth.double().requires_grad_(True), mask.double().requires_grad_(True)
    loss, pred = R.torch_tail(d64, m64, gt.double().unsqueeze(1), valid.unsqueeze(1))
    (loss * 3.0).backward()
    ref = R.dnet_loss_ref(depth, mask, gt, valid, grad_loss=3.0)
    assert ref["count"] == int(valid.sum()) > 0
    np.testing.assert_allclose(ref["pred"].numpy(), pred.detach().numpy(), rtol=1e-13, atol=0)
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-13 * max(abs(float(loss.detach())), 1.0)
    # two float64 evaluations of the same sums in another order: they differ by float64 roundings of terms of the gradients' size
    for name, got in (("grad_depth", d64.grad), ("grad_mask", m64.grad)):
        scale = float(got.abs().max())
        np.testing.assert_allclose(ref[name].numpy(), got.numpy(), rtol=1e-10, atol=1e-12 * scale, err_msg=name)


def _ratios(em, ref):
    return dict(pred=R.worst_ratio(torch.from_numpy(em["pred"]), ref["pred"], ref["bound_pred"]),
                loss=abs(em["loss"] - ref["loss"]) / ref["bound_loss"],
                grad_depth=R.worst_ratio(torch.from_numpy(em["grad_depth"]), ref["grad_depth"], ref["bound_grad_depth"]),
                grad_mask=R.worst_ratio(torch.from_numpy(em["grad_mask"]), ref["grad_mask"], ref["bound_grad_mask"]))


@pytest.mark.parametrize("shape,std", [((2, 13, 17), 1.0), ((2, 13, 17), 8.0), ((1, 1, 1), 1.0), ((1, 2, 67), 8.0), ((1, 5, 1), 30.0)])
def test_bounds_hold_for_the_fp32_emulation(shape, std):
    depth, mask, gt, valid = R.random_case(*shape, std, seed=7 * sum(shape) + int(std))
    ref = R.dnet_loss_ref(depth, mask, gt, valid, grad_loss=2.0)
    em = R.emulate_fp32(depth.numpy(), mask.numpy(), gt.numpy(), valid.numpy(), grad_loss=2.0)
    r = _ratios(em, ref)
    print(f"{shape} std {std}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert max(r.values()) > 1e-3                                           # the bounds are not vacuous


@pytest.mark.parametrize("pattern", ["v_floor", "v_positive", "mu_equals_gt", "one_tap_1e4", "spread_88", "equal"])
def test_bounds_hold_for_the_fp32_emulation_on_patterns(pattern):
    depth, mask, gt, valid = R.random_case(2, 5, 7, 1.0, seed=len(pattern))
    depth, mask, gt = R.pattern_case(pattern, depth, mask, gt)
    ref = R.dnet_loss_ref(depth, mask, gt, valid)
    em = R.emulate_fp32(depth.numpy(), mask.numpy(), gt.numpy(), valid.numpy())
    r = _ratios(em, ref)
    print(f"{pattern}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert np.isfinite(em["grad_mask"]).all() and np.isfinite(em["grad_depth"]).all() and np.isfinite(em["loss"])
    if pattern == "v_floor":
        assert (em["pred"][:, 1] >= np.float32(1e-10)).all()
        assert (em["pred"][:, 1, 4:-4, 4:-4] < 1e-7).all()                  # away from the border, where the zero neighbours pull vu up


def test_wrong_gradients_exceed_the_bounds():
    """Negative controls: the ELU derivative taken as 1 below zero, and the neighbour offset of grad_depth with its sign flipped."""
    depth, mask, gt, valid = R.random_case(2, 13, 17, 1.0, seed=38)
    ref = R.dnet_loss_ref(depth, mask, gt, valid)
    assert float((depth[:, 1] < 0).float().mean()) > 0.3
    wrong = R.dnet_loss_ref(depth, mask, gt, valid, elu_grad_one=True)
    r_d = R.worst_ratio(wrong["grad_depth"], ref["grad_depth"], ref["bound_grad_depth"])
    r_m = R.worst_ratio(wrong["grad_mask"], ref["grad_mask"], ref["bound_grad_mask"])
    print(f"ELU derivative 1: grad_depth {r_d:.3g} x its bound, grad_mask {r_m:.3g} x")
    assert r_d > 1.0 and r_m > 1.0
    wrong = R.dnet_loss_ref(depth, mask, gt, valid, flip_offsets=True)
    r_d = R.worst_ratio(wrong["grad_depth"], ref["grad_depth"], ref["bound_grad_depth"])
    print(f"flipped offsets: grad_depth {r_d:.3g} x its bound")
    assert r_d > 1.0
    assert torch.equal(wrong["grad_mask"], ref["grad_mask"])                # the flip touches grad_depth alone


def test_plain_form_and_its_clamp_against_float64_autograd():
    pred, gt, valid, ns = R.plain_case()
    p64 = pred.double().requires_grad_(True)
    loss = R.reference_loss(p64, gt.double().unsqueeze(1), valid.unsqueeze(1))
    (loss * 0.5).backward()
    ref = R.dnet_nll_ref(pred, gt, valid, grad_loss=0.5)
    assert ref["count"] == int(valid.sum())
    assert ref["clamped"][0, 0, :ns].tolist() == [True, True, True, True, False, False, True]
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-13 * abs(float(loss.detach()))
    np.testing.assert_allclose(ref["grad"].numpy(), p64.grad.numpy(), rtol=1e-12, atol=0)
    assert not ref["grad"][:, 1][ref["clamped"]].any()                      # no var gradient where the clamp applied
    assert ref["grad"][:, 0][ref["clamped"] & valid].abs().min() > 0        # mu keeps its gradient there
    assert not ref["grad"].permute(1, 0, 2, 3)[:, ~valid].any()           # nothing outside the mask


def test_new_symbols_are_declared_and_exported(hip_lib):
    text = open(HEADER).read()
    for name, struct in (("magnet_dnet_loss_forward", "MagnetDnetLossArgs"), ("magnet_dnet_loss_backward", "MagnetDnetLossArgs"),
                         ("magnet_dnet_nll_forward", "MagnetDnetNllArgs"), ("magnet_dnet_nll_backward", "MagnetDnetNllArgs")):
        assert name in lib.API_SYMBOLS and name in lib._PROTOS and hasattr(hip_lib, name)
        assert re.search(r"MAGNET_API int %s\(const %s \*args, void \*stream\);" % (name, struct), text)
    assert "magnet_dnet_loss_workspace" in lib._PROTOS and hasattr(hip_lib, "magnet_dnet_loss_workspace")
    assert re.search(r"MAGNET_API int64_t magnet_dnet_loss_workspace\(const MagnetDnetLossArgs \*args\);", text)
    assert re.search(r"#define MAGNET_HIP_VERSION 500\b", text)              # the header's literal is the library's
    assert list(lib._PROTOS)[-5:] == ["magnet_dnet_loss_workspace", "magnet_dnet_loss_forward", "magnet_dnet_loss_backward",
                                      "magnet_dnet_nll_forward", "magnet_dnet_nll_backward"]


def test_entry_points_return_codes(hip_lib):
    L = hip_lib
    fwd, bwd, ws = L.magnet_dnet_loss_forward, L.magnet_dnet_loss_backward, L.magnet_dnet_loss_workspace
    assert fwd(None, None) == lib.E_NULL and bwd(None, None) == lib.E_NULL and ws(None) == -lib.E_NULL
    a = lib.MagnetDnetLossArgs()
    assert fwd(ctypes.byref(a), None) == lib.E_NULL and b"NULL" in L.magnet_last_error()
    a.depth = a.mask = a.gt = a.valid = a.sums = a.work = a.loss = 16
    a.B, a.h, a.w, a.k = 2, 120, 160, 8
    assert fwd(ctypes.byref(a), None) == lib.E_DIM and b"k=8" in L.magnet_last_error()
    assert ws(ctypes.byref(a)) == -lib.E_DIM
    a.k = 4
    assert ws(ctypes.byref(a)) == 2 * 120 * 160 * 18 * 4                    # the backward's tap sums: 18 floats per coarse pixel
    for f in ("B", "h", "w"):
        old = getattr(a, f); setattr(a, f, 0)
        assert fwd(ctypes.byref(a), None) == lib.E_DIM and bwd(ctypes.byref(a), None) == lib.E_DIM and ws(ctypes.byref(a)) == -lib.E_DIM
        setattr(a, f, -3)
        assert fwd(ctypes.byref(a), None) == lib.E_DIM
        setattr(a, f, old)
    a.B, a.h, a.w = 1, 1, 1
    assert ws(ctypes.byref(a)) == 18 * 4
    a.gt = 20
    assert fwd(ctypes.byref(a), None) == lib.E_ALIGN
    a.gt = 16; a.valid = 18
    assert fwd(ctypes.byref(a), None) == lib.E_ALIGN
    a.valid = 16; a.loss = None
    assert fwd(ctypes.byref(a), None) == lib.E_NULL
    assert bwd(ctypes.byref(a), None) == lib.E_NULL                         # grad_loss, grad_depth, grad_mask
    a.grad_loss = a.grad_depth = 16
    assert bwd(ctypes.byref(a), None) == lib.E_NULL
    a.grad_mask = 16; a.work = None
    assert bwd(ctypes.byref(a), None) == lib.E_NULL
    pf, pb = L.magnet_dnet_nll_forward, L.magnet_dnet_nll_backward
    assert pf(None, None) == lib.E_NULL and pb(None, None) == lib.E_NULL
    n = lib.MagnetDnetNllArgs()
    assert pf(ctypes.byref(n), None) == lib.E_NULL
    n.pred = n.gt = n.valid = n.sums = n.loss = n.work = 16
    n.B, n.H, n.W = 1, 0, 4
    assert pf(ctypes.byref(n), None) == lib.E_DIM and b"H=0" in L.magnet_last_error()
    n.H = 4
    assert pb(ctypes.byref(n), None) == lib.E_NULL                          # grad_loss, grad_pred
    n.grad_loss = n.grad_pred = 16; n.W = -1
    assert pb(ctypes.byref(n), None) == lib.E_DIM


def _args(**kw):
    a = dict(loss_fn="gaussian"); a.update(kw)
    return SimpleNamespace(**a)


def test_dnet_loss_rejects_bad_arguments():
    depth, mask = torch.zeros(2, 2, 3, 5), torch.zeros(2, 144, 3, 5)
    gt, valid = torch.ones(2, 1, 12, 20), torch.ones(2, 1, 12, 20, dtype=torch.bool)
    pred = torch.ones(2, 2, 12, 20)
    crit = DnetLoss(_args())
    assert crit.pred is None
    for out in (pred, (depth, mask)):
        with pytest.raises(lib.MagnetError, match="GPU tensor"):
            crit(out, gt, valid)
        with pytest.raises(lib.MagnetError, match="loss_fn 'l1'"):
            DnetLoss(_args(loss_fn="l1"))(out, gt, valid)
        with pytest.raises(lib.MagnetError, match="expected"):
            crit(out, gt[:, 0], valid)                                      # (B, H, W)
        with pytest.raises(lib.MagnetError, match="expected"):
            crit(out, gt, valid[:1])
        with pytest.raises(lib.MagnetError, match="expected"):
            crit(out, gt[..., :19], valid[..., :19])
    with pytest.raises(lib.MagnetError, match="144"):
        crit((depth, mask[:, :143]), gt, valid)
    with pytest.raises(lib.MagnetError, match="144"):
        crit((depth, torch.zeros(2, 144, 3, 4)), gt, valid)
    with pytest.raises(lib.MagnetError, match=r"\(B,2,h,w\)"):
        crit((depth[:, :1], mask), gt, valid)
    with pytest.raises(lib.MagnetError, match=r"\(B,2,H,W\)"):
        crit(pred[:, :1], gt, valid)
    with pytest.raises(lib.MagnetError, match="torch.Tensor"):
        crit((depth, None), gt, valid)
    with pytest.raises(lib.MagnetError, match=r"\(depth, up_mask\)"):
        crit((depth, mask, mask), gt, valid)
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        lib.dnet_loss_forward(depth, mask, gt[:, 0], valid[:, 0])
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        lib.dnet_nll_forward(pred, gt[:, 0], valid[:, 0])


def test_dnet_forward_without_upsampling_returns_the_raw_pair():
    img = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(0))
    model = make_dnet(dnet=True)
    with torch.no_grad():
        depth, up_mask = model(img, upsample=False)
        assert tuple(depth.shape) == (2, 2, 16, 24) and tuple(up_mask.shape) == (2, 144, 16, 24)
        full = model(img)
        assert tuple(full.shape) == (2, 2, 64, 96)
        assert torch.equal(full, model(img, upsample=True))                 # the default call is unchanged
        tail = R.torch_tail(depth, up_mask, torch.ones(2, 1, 64, 96), torch.ones(2, 1, 64, 96, dtype=torch.bool))[1]
        assert torch.equal(full, tail)                                      # the raw pair is what the torch tail consumes
        feats = model.d_net.encoder(img)
        assert torch.equal(model.d_net.decoder(feats), model.d_net.decoder(feats, upsample=True))
    with pytest.raises(lib.MagnetError, match="dnet=True"):
        make_dnet(dnet=False)(img, upsample=False)
    with pytest.raises(lib.MagnetError, match="dnet=True"):
        DNET(make_dnet_args(), StandinEncoder(), dnet=False).d_net(img, upsample=False)      # the decoder's own check
    mono, x_feat = make_dnet(dnet=False)(img)                               # MaGNet's D-Net keeps its pair
    assert tuple(mono.shape) == (2, 2, 16, 24) and tuple(x_feat.shape) == (2, 256, 16, 24)
    hip = DNET(make_dnet_args(), StandinEncoder(), dnet=True, backend="hip").train()
    with torch.no_grad():
        d2, m2 = hip(img, upsample=False)                                   # torch modules on either backend
    assert tuple(d2.shape) == (2, 2, 16, 24) and tuple(m2.shape) == (2, 144, 16, 24)
