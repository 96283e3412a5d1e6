"""Training losses (reference utils/losses.py).  MagnetLoss is the loss of train_MaGNet.py:87-98 on HIP kernels
(csrc/train_bwd.hip); DnetLoss is out of scope with the D-Net."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import lib


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
