"""Training losses (reference utils/losses.py and the inline loss of train_FNet.py).  MagnetLoss is the loss of train_MaGNet.py:87-98
on HIP kernels (csrc/train_bwd.hip); FnetLoss is the tail of the F-Net step, train_FNet.py:95-104 (softmax over the bins, expected
depth, masked L1), fused on HIP kernels (csrc/fnet_loss.hip); DnetLoss is the loss of train_DNet.py (utils/losses.py:8-24), either on
the upsampled prediction as the reference calls it or fused with the stand-alone D-Net's tail behind the two head convolutions
(learned convex upsampling, activation_G, NLL; csrc/dnet_loss.hip)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lib
from .homography import d_center_device


class _GaussianNLL(torch.autograd.Function):
    """sum_i gamma^(n-1-i) mean_mask[(mu_i - gt)^2 / (2 var_i) + 0.5 log var_i], var_i = max(sigma_i^2, 1e-10) (no gradient where
    clamped).  Forward: a deterministic two-stage reduction; backward: reads grad_output on the device (no host sync)."""

    @staticmethod
    def forward(ctx, gamma, gt, mask, *preds):
        P = torch.stack([p.detach().float() for p in preds]).contiguous()
        loss, sums = lib.nll_loss_forward(P, gt, mask, gamma)
        ctx.gamma, ctx.n = gamma, len(preds)
        ctx.save_for_backward(P, gt, mask, sums)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        P, gt, mask, sums = ctx.saved_tensors
        g = lib.nll_loss_backward(P, gt, mask, sums, grad_out.float().reshape(()).contiguous(), ctx.gamma)
        return (None, None, None, *g.unbind(0))


class MagnetLoss(nn.Module):
    """Drop-in for the reference's utils.losses.MagnetLoss (utils/losses.py:28-52): reads args.loss_fn and args.loss_gamma;
    forward(pred_list, gt_depth (B,1,H,W), gt_depth_mask (B,1,H,W) bool) -> 0-d tensor.  Only loss_fn 'gaussian' exists, as in
    the reference.  Accepts the predictions of either training backend; GPU tensors only (no CPU fallback)."""

    def __init__(self, args):
        super().__init__()
        self.loss_type = args.loss_fn
        self.gamma = args.loss_gamma

    def forward(self, pred_list, gt_depth, gt_depth_mask):
        if self.loss_type != "gaussian":
            raise lib.MagnetError(f"MagnetLoss: loss_fn {self.loss_type!r} is not supported (the reference has 'gaussian' only)")
        preds = list(pred_list)
        if not preds:
            raise lib.MagnetError("MagnetLoss: empty pred_list")
        for t, name in [(p, "pred_list[%d]" % i) for i, p in enumerate(preds)] + [(gt_depth, "gt_depth"), (gt_depth_mask, "gt_depth_mask")]:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise lib.MagnetError(f"MagnetLoss: {name} must be a GPU tensor (magnet_amd has no CPU fallback)")
        B, C, H, W = preds[0].shape
        if C != 2 or any(tuple(p.shape) != (B, 2, H, W) for p in preds):
            raise lib.MagnetError("MagnetLoss: every prediction must be (B, 2, H, W)")
        gt = gt_depth.detach().float().reshape(B, H, W).contiguous()
        mask = gt_depth_mask.detach().reshape(B, H, W).bool().contiguous()
        return _GaussianNLL.apply(float(self.gamma), gt, mask, *preds)


class _FnetL1(torch.autograd.Function):
    """mean over the valid pixels of |sum_j softmax(raw)_j d_j - gt| and the detached expected depth, from the raw volume in one pass;
    backward: one read of raw, one write of its gradient (closed form), grad_output read on the device (no host sync).  The gradient is
    a fresh contiguous tensor: the cost volume's backward takes it as it is."""

    @staticmethod
    def forward(ctx, raw, d, gt, min_depth, max_depth):
        x = raw.detach()
        loss, pred, m, rz, sums = lib.fnet_loss_forward(x, d, gt, min_depth, max_depth)
        ctx.depths = (min_depth, max_depth)
        ctx.save_for_backward(x, d, gt, pred, m, rz, sums)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_pred):
        x, d, gt, pred, m, rz, sums = ctx.saved_tensors
        g = lib.fnet_loss_backward(x, d, gt, pred, m, rz, sums, grad_out.float().reshape(()).contiguous(), *ctx.depths)
        return g, None, None, None, None


class FnetLoss(nn.Module):
    """The loss of the reference's F-Net driver (train_FNet.py:95-104) on the RAW volume of MAGNET_F(..., softmax=False):
    reads args.loss_fn (only 'l1' exists, as in the reference), args.min_depth and args.max_depth;
    forward(raw_volume (B,D,h,w), d_center (D bins, any shape), gt_dmap (B,1,H,W)) -> 0-d tensor.  A gt_dmap of another resolution is
    brought to the volume's with F.interpolate(mode='nearest') as the driver does; pixels with gt > max_depth or gt <= min_depth do not
    count (the driver's gt[gt > max_depth] = 0 commutes with nearest sampling, so gt_dmap may come clipped or not).
    pred_dmap: the detached (B,1,h,w) expected depth of the last forward (visualize_F, the progress line).  GPU tensors only."""

    def __init__(self, args):
        super().__init__()
        self.loss_type = args.loss_fn
        self.min_depth = float(args.min_depth)
        self.max_depth = float(args.max_depth)
        self.pred_dmap = None

    def forward(self, raw_volume, d_center, gt_dmap):
        if self.loss_type != "l1":
            raise lib.MagnetError(f"FnetLoss: loss_fn {self.loss_type!r} is not supported (the reference has 'l1' only)")
        for t, name in ((raw_volume, "raw_volume"), (d_center, "d_center"), (gt_dmap, "gt_dmap")):
            if not isinstance(t, torch.Tensor):
                raise lib.MagnetError(f"FnetLoss: {name} must be a torch.Tensor, got {type(t).__name__}")
        if raw_volume.dim() != 4 or gt_dmap.dim() != 4 or gt_dmap.shape[0] != raw_volume.shape[0] or gt_dmap.shape[1] != 1:
            raise lib.MagnetError(f"FnetLoss: raw_volume {tuple(raw_volume.shape)} / gt_dmap {tuple(gt_dmap.shape)}, expected (B,D,h,w) and (B,1,H,W)")
        B, D, h, w = raw_volume.shape
        if d_center.numel() != D:
            raise lib.MagnetError(f"FnetLoss: d_center has {d_center.numel()} bins, raw_volume has D = {D}")
        if not 1 <= D <= lib.MAX_CANDIDATES:
            raise lib.MagnetError(f"FnetLoss: 1 <= D <= {lib.MAX_CANDIDATES}, got {D}")
        if self.min_depth < 0:
            raise lib.MagnetError(f"FnetLoss: min_depth must be >= 0, got {self.min_depth}")
        for t, name in ((raw_volume, "raw_volume"), (gt_dmap, "gt_dmap")):
            if not t.is_cuda:
                raise lib.MagnetError(f"FnetLoss: {name} must be a GPU tensor (magnet_amd has no CPU fallback)")
        gt = gt_dmap.detach().float()
        if tuple(gt.shape[2:]) != (h, w):
            gt = F.interpolate(gt, size=[h, w], mode="nearest")               # train_FNet.py:98
        x = raw_volume if raw_volume.dtype == torch.float32 and raw_volume.is_contiguous() else raw_volume.float().contiguous()
        loss, pred = _FnetL1.apply(x, d_center_device(d_center, x.device), gt.reshape(B, h, w).contiguous(), self.min_depth, self.max_depth)
        self.pred_dmap = pred.unsqueeze(1)
        return loss


class _DnetNll(torch.autograd.Function):
    """mean over the valid pixels of (mu - gt)^2 / (2 var) + 0.5 log var on pred (B,2,H,W) [mu, var], var clamped to 1e-10 (no var
    gradient where clamped); backward reads grad_output on the device (no host sync)."""

    @staticmethod
    def forward(ctx, pred, gt, valid):
        p = pred.detach()
        loss, sums = lib.dnet_nll_forward(p, gt, valid)
        ctx.save_for_backward(p, gt, valid, sums)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        p, gt, valid, sums = ctx.saved_tensors
        return lib.dnet_nll_backward(p, gt, valid, sums, grad_out.float().reshape(()).contiguous()), None, None


class _DnetTail(torch.autograd.Function):
    """The loss from the raw head output and the mask logits in one pass, and the detached (B,2,4h,4w) [mu, var]; the backward
    recomputes the softmax from the logits (only the inputs and the two fp64 sums are saved), reads grad_output on the device and
    returns the gradients of both inputs."""

    @staticmethod
    def forward(ctx, depth, up_mask, gt, valid):
        d, m = depth.detach(), up_mask.detach()
        loss, sums, pred = lib.dnet_loss_forward(d, m, gt, valid)
        ctx.save_for_backward(d, m, gt, valid, sums)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_pred):
        d, m, gt, valid, sums = ctx.saved_tensors
        gd, gm = lib.dnet_loss_backward(d, m, gt, valid, sums, grad_out.float().reshape(()).contiguous())
        return gd, gm, None, None


class DnetLoss(nn.Module):
    """Drop-in for the reference's utils.losses.DnetLoss (utils/losses.py:8-24): reads args.loss_fn (only 'gaussian' exists, as in the
    reference).  forward(out, gt_depth (B,1,H,W), gt_depth_mask (B,1,H,W) bool) -> 0-d tensor, with
      out = pred (B,2,H,W) [mu, var]: the reference's call on the upsampled prediction, or
      out = (depth (B,2,h,w), up_mask (B,144,h,w)), what DNET(dnet=True)(img, upsample=False) returns: the tail of the step fused
            (upsample_depth_via_mask, activation_G and the loss in one pass over the logits; H = 4h, W = 4w).  After such a call
            `pred` is the detached (B,2,H,W) [mu, var] (visualize_D, the progress line).
    Inputs that are not fp32 (the mask may be channel-last) are brought to fp32; GPU tensors only (no CPU fallback)."""

    def __init__(self, args):
        super().__init__()
        self.loss_type = args.loss_fn
        self.pred = None

    def forward(self, out, gt_depth, gt_depth_mask):
        if self.loss_type != "gaussian":
            raise lib.MagnetError(f"DnetLoss: loss_fn {self.loss_type!r} is not supported (the reference has 'gaussian' only)")
        fused = isinstance(out, (tuple, list))
        if fused and len(out) != 2:
            raise lib.MagnetError("DnetLoss: the fused form takes (depth, up_mask)")
        tensors = [(out[0], "depth"), (out[1], "up_mask")] if fused else [(out, "pred")]
        for t, name in tensors + [(gt_depth, "gt_depth"), (gt_depth_mask, "gt_depth_mask")]:
            if not isinstance(t, torch.Tensor):
                raise lib.MagnetError(f"DnetLoss: {name} must be a torch.Tensor, got {type(t).__name__}")
        first = tensors[0][0]
        if first.dim() != 4 or first.shape[1] != 2:
            raise lib.MagnetError(f"DnetLoss: {tensors[0][1]} {tuple(first.shape)}, expected (B,2,{'h,w' if fused else 'H,W'})")
        B, _, h, w = first.shape
        H, W = (4 * h, 4 * w) if fused else (h, w)
        if fused and tuple(out[1].shape) != (B, 144, h, w):
            raise lib.MagnetError(f"DnetLoss: up_mask {tuple(out[1].shape)}, expected {(B, 144, h, w)} (9 taps x 4 x 4 sub-pixels)")
        if tuple(gt_depth.shape) != (B, 1, H, W) or tuple(gt_depth_mask.shape) != (B, 1, H, W):
            raise lib.MagnetError(f"DnetLoss: gt_depth {tuple(gt_depth.shape)} / gt_depth_mask {tuple(gt_depth_mask.shape)}, "
                                  f"expected {(B, 1, H, W)}")
        for t, name in tensors + [(gt_depth, "gt_depth"), (gt_depth_mask, "gt_depth_mask")]:
            if not t.is_cuda:
                raise lib.MagnetError(f"DnetLoss: {name} must be a GPU tensor (magnet_amd has no CPU fallback)")
        gt = gt_depth.detach().float().reshape(B, H, W).contiguous()
        valid = gt_depth_mask.detach().reshape(B, H, W).bool().contiguous()
        f32 = lambda t: t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()
        if not fused:
            return _DnetNll.apply(f32(out), gt, valid)
        mask = out[1]
        if mask.dtype != torch.float32 or not (mask.is_contiguous() or mask.is_contiguous(memory_format=torch.channels_last)):
            mask = mask.float().contiguous()
        loss, self.pred = _DnetTail.apply(f32(out[0]), mask, gt, valid)
        return loss
