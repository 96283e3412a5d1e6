"""The HIP training path of g_net and mask_head (MAGNET(..., train_backend="hip"); reference train_MaGNet.py:87-98).

Forward (no new kernel): each stack runs layer by layer on lib.conv_mfma, so the post-ReLU activations h1, h2, h3 stay on the
device as split-bf16 (hi, lo) planes of the zero-bordered channel-last grid for the backward; G-Net's first layer is split as at
inference (x_d3 part once per forward, the round_up(D, 32) cost channels per iteration); the Gaussian update and the upsampling are
the inference kernels.  Backward (csrc/train_bwd.hip): convex-upsampling backward -> per stack one dgrad launch through the 1x1
tail (G-Net's starts at the Gaussian update) -> weight gradients on the matrix cores.  The reference detaches the matcher's
inputs and every iteration's G-Net input (models/MAGNET.py:154,167-168), so each iteration's backward is local and the first
layers need no input gradient; the x_d3 part of G-Net's first layer gets ONE weight gradient with sum_i dh1_i.

Memory kept for the backward per frame, P = (h+2)(w+2) grid rows: G-Net P x (3 x 128 x 4 B (h1..h3, hi + lo) + 32 x 4 B (cost
copy) + 16 x 4 B (head output)) per iteration; mask head P x (3 x 128 x 4 B + 144 x 4 B); the input buffer P x 320 x 4 B.  At
120 x 160 (P = 19 764): 34 MB per frame and iteration for G-Net, 42 MB mask head, 25 MB input: 169 MB per frame at I = 3.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import lib
from .convnet import ConvStackMFMA
from .planes import planes, round_up, split_bf16

# the zero-bordered channel-last grid one stack runs on: B frames of (h+2) x (w+2) = wp rows
_Grid = namedtuple("_Grid", "B h w rows wp dev")


def _split_t(wt_list):
    """[W4^T | W3^T | W2^T] as flat split-bf16 planes for magnet_head_dgrad."""
    return split_bf16(torch.cat([w.reshape(-1) for w in wt_list]).contiguous())


def _transposed(packs, k0):
    """The forward's packed 1x1 weights (hi + lo = the exact values the kernels multiplied by) transposed for the dgrad."""
    out = []
    for li, kk in ((3, k0), (2, 128), (1, 128)):
        w = packs[li]["w_hi"].float()[0] + packs[li]["w_lo"].float()[0]          # (cout_pad, 128)
        wt = torch.zeros((128, kk), dtype=torch.float32, device=w.device)
        wt[:, :min(w.shape[0], kk)] = w.t()[:, :kk]
        out.append(wt)
    return _split_t(out)


def _params(model):
    mods = [model.g_net.gnet[i] for i in (0, 2, 4, 6)] + [model.mask_head[i] for i in (0, 2, 4, 6)]
    out = []
    for m in mods:
        out += [m.weight, m.bias]
    return out


def _stack_forward(grid, packs, x, in_ld, first=None, addend=None):
    """One packed stack (3x3 + three 1x1) layer by layer on the planes x = (hi, lo) of pitch in_ld: ([h1, h2, h3] post-ReLU split
    planes, fp32 output (rows, cout_pad)).  first: the pack that takes the first layer's place; addend: fp32 (rows, 128) added to it."""
    rows, wp, dev = grid.rows, grid.wp, grid.dev
    hs = []
    for li in range(3):
        pk = first if li == 0 and first is not None else packs[li]
        o = planes(rows, 128, dev)
        lib.conv_mfma(x[0], x[1], in_ld, pk["cin"], pk["w_hi"], pk["w_lo"], pk["bias"], pk["taps"], wp, True, rows,
                      out_hi=o[0], out_lo=o[1], addend=addend if li == 0 else None)
        hs.append(o)
        x, in_ld = o, 128
    pk = packs[3]
    out = torch.empty((rows, pk["cout_pad"]), dtype=torch.float32, device=dev)
    lib.conv_mfma(x[0], x[1], 128, pk["cin"], pk["w_hi"], pk["w_lo"], pk["bias"], 1, wp, False, rows, out_f32=out)
    return hs, out


def _dgrad(grid, dout, k0, wt, hs, acc=None, acc_mode=0, acc_planes=None, gauss=None):
    """The one magnet_head_dgrad launch of a stack: (dout, dh3, dh2, dh1) split planes."""
    rows, dev = grid.rows, grid.dev
    dout_p = planes(rows, k0, dev)
    d3, d2, d1 = planes(rows, 128, dev), planes(rows, 128, dev), planes(rows, 128, dev)
    a = lib.MagnetHeadDgradArgs(
        dout=dout.data_ptr() if dout is not None else None, k0=k0, wt_hi=wt[0].data_ptr(), wt_lo=wt[1].data_ptr(),
        h3_hi=hs[2][0].data_ptr(), h2_hi=hs[1][0].data_ptr(), h1_hi=hs[0][0].data_ptr(),
        dout_hi=dout_p[0].data_ptr(), dout_lo=dout_p[1].data_ptr(), dh3_hi=d3[0].data_ptr(), dh3_lo=d3[1].data_ptr(),
        dh2_hi=d2[0].data_ptr(), dh2_lo=d2[1].data_ptr(), dh1_hi=d1[0].data_ptr(), dh1_lo=d1[1].data_ptr(),
        acc=acc.data_ptr() if acc is not None else None,
        acc_hi=acc_planes[0].data_ptr() if acc_planes is not None else None,
        acc_lo=acc_planes[1].data_ptr() if acc_planes is not None else None, acc_mode=acc_mode,
        B=grid.B, h=grid.h, w=grid.w, rows=rows)
    if gauss is not None:
        gg, out, gmm_in = gauss
        gg = gg.contiguous()
        a.grad_gmm, a.gnet_out, a.gmm_in, a.gnet_ld = gg.data_ptr(), out.data_ptr(), gmm_in.data_ptr(), out.shape[1]
    lib.head_dgrad(a, dev)
    return dout_p, d3, d2, d1


def _tail_wgrads(grid, dh, hs, g, cout_last, accumulate):
    """Weight / bias gradients of the three 1x1 layers; g = [W1, b1, W2, b2, W3, b3, W4, b4] of the stack."""
    rows, wp = grid.rows, grid.wp
    dout_p, d3, d2, _ = dh
    lib.wgrad(dout_p[0], dout_p[1], hs[2][0], hs[2][1], rows, wp, 1, round_up(cout_last, 8), 128, g[6], cout_valid=cout_last,
              grad_b=g[7], accumulate=accumulate)
    lib.wgrad(d3[0], d3[1], hs[1][0], hs[1][1], rows, wp, 1, 128, 128, g[4], grad_b=g[5], accumulate=accumulate)
    lib.wgrad(d2[0], d2[1], hs[0][0], hs[0][1], rows, wp, 1, 128, 128, g[2], grad_b=g[3], accumulate=accumulate)


def _stack_backward(grid, dout, k0, wt, hs, g, x, cin, cin_dst, cout_last):
    dh = _dgrad(grid, dout, k0, wt, hs)
    _tail_wgrads(grid, dh, hs, g, cout_last, accumulate=False)
    lib.wgrad(dh[3][0], dh[3][1], x[0], x[1], grid.rows, grid.wp, 9, 128, cin, g[0], cin_dst=cin_dst, grad_b=g[1])


class _Runner:
    """State of one HIP training forward (buffers the backward reads)."""

    def __init__(self, model, matcher, ref_gmms, x_d3, n_iter):
        self.model, self.matcher, self.ref_gmms, self.x_d3, self.n_iter = model, matcher, ref_gmms, x_d3, n_iter

    @torch.no_grad()
    def forward(self):
        m = self.model
        B, _, h, w = self.ref_gmms.shape
        D = m.n_samples
        dev = self.ref_gmms.device
        _, _, ctot, Dp = m.gnet_input_buffer(B, h, w, dev)          # builds the stacks (the cached inference buffer is not used)
        g_stack, m_stack = m._stacks
        rows, wp = B * (h + 2) * (w + 2), w + 2
        cv = round_up(D, 32)
        self.B, self.h, self.w, self.D, self.Dp, self.ctot, self.rows, self.wp, self.cv = B, h, w, D, Dp, ctot, rows, wp, cv
        grid = self.grid = _Grid(B, h, w, rows, wp, dev)
        # a fresh input buffer per forward: the backward reads its x_d3 channels, whatever runs in between
        gin_hi = torch.zeros((rows, ctot), dtype=torch.bfloat16, device=dev)
        gin_lo = torch.zeros((rows, ctot), dtype=torch.bfloat16, device=dev)
        self.gin = (gin_hi, gin_lo)
        lib.pack_split(self.x_d3.detach().float().contiguous(), gin_hi, gin_lo, ctot, Dp)
        gp, mp = g_stack.packed(dev), m_stack.packed(dev)
        var, inv = g_stack.packed_first_split(dev, D, Dp)
        self.gp, self.mp = gp, mp
        # loop-invariant x_d3 part of G-Net's first layer (K = 9 * 256), once per forward
        partial = torch.empty((rows, 128), dtype=torch.float32, device=dev)
        lib.conv_mfma(gin_hi[:, Dp:], gin_lo[:, Dp:], ctot, inv["cin"], inv["w_hi"], inv["w_lo"], inv["bias"], inv["taps"], wp,
                      False, rows, out_f32=partial)
        cost_nchw = None
        split_out = m.matcher_path in (0, 2, 4)
        pred_list = [self.ref_gmms.detach().float().contiguous()]
        self.iters = []
        for _ in range(self.n_iter):
            if split_out:
                try:
                    self.matcher(ref_gmm=pred_list[-1], k_list=m.k_list, out_split=(gin_hi, gin_lo, ctot))   # MAGNET.py:153-164
                except lib.MagnetError as e:
                    if e.code != lib.E_SHAPE:
                        raise
                    split_out = False
            if not split_out:
                if cost_nchw is None:
                    cost_nchw = torch.empty((B, D, h, w), dtype=torch.float32, device=dev)
                self.matcher(ref_gmm=pred_list[-1], k_list=m.k_list, out=cost_nchw)
                lib.pack_split(cost_nchw, gin_hi, gin_lo, ctot, 0)
            it = {"cost": (gin_hi[:, :cv].clone(), gin_lo[:, :cv].clone()), "gmm_in": pred_list[-1]}
            it["h"], it["out"] = _stack_forward(grid, gp, self.gin, ctot, first=var, addend=partial)  # MAGNET.py:51-56,62
            pred_list.append(lib.gaussian_update_cl(it["out"], gp[3]["cout_pad"], pred_list[-1], h, w))  # MAGNET.py:60-69
            self.iters.append(it)
        # mask head (MAGNET.py:172) on the x_d3 channels of the same buffer
        self.mh, self.mask = _stack_forward(grid, mp, (gin_hi[:, Dp:], gin_lo[:, Dp:]), ctot)
        self.mask_ld = mp[3]["cout_pad"]
        self.preds = pred_list[1:]
        return lib.upsample_depth_cl_n(self.preds, self.mask, self.mask_ld)                         # MAGNET.py:173

    @torch.no_grad()
    def backward(self, grad_ups):
        m = self.model
        grid, D, Dp, cv = self.grid, self.D, self.Dp, self.cv
        B, h, w, rows, wp, dev = grid
        gin_hi, gin_lo = self.gin
        params = _params(m)
        grads = [torch.zeros(p.shape, dtype=torch.float32, device=dev) for p in params]
        # ---- convex upsampling backward: d pred_i and d mask (summed over the iterations) ----
        gup = torch.stack([g.float() for g in grad_ups]).contiguous()
        preds = torch.stack(self.preds).contiguous()
        ld, mk = self.mask_ld, 160
        dmask = torch.zeros((rows, mk), dtype=torch.float32, device=dev)
        pg = (h + 2) * wp
        d_preds, _ = lib.upsample_depth_backward(gup, preds, self.mask, m.downsample_ratio,
                                                 mask_layout=((wp + 1) * ld, pg * ld, 1, wp * ld, ld), grad_mask=dmask,
                                                 grad_mask_layout=((wp + 1) * mk, pg * mk, 1, wp * mk, mk))
        # ---- mask head ----
        mwt = _transposed(self.mp, mk)
        _stack_backward(grid, dmask, mk, mwt, self.mh, grads[8:16], (gin_hi[:, Dp:], gin_lo[:, Dp:]), 256, 0,
                        m.mask_head[6].out_channels)
        # ---- G-Net, iteration by iteration (each iteration's backward is local: MAGNET.py:168 detaches pred_list[-1]) ----
        gwt = _transposed(self.gp, 32)
        acc = torch.empty((rows, 128), dtype=torch.float32, device=dev)
        acc_planes = planes(rows, 128, dev)
        n = len(self.iters)
        for i, it in enumerate(self.iters):
            last = i == n - 1
            dh = _dgrad(grid, None, 32, gwt, it["h"], acc=acc, acc_mode=1 if i == 0 else 2, acc_planes=acc_planes if last else None,
                        gauss=(d_preds[i], it["out"], it["gmm_in"]))
            _tail_wgrads(grid, dh, it["h"], grads[0:8], cout_last=2, accumulate=i > 0)
            # first layer, cost channels (buffer channels [0, D) -> nn.Conv2d input channels [0, D)), per iteration
            lib.wgrad(dh[3][0], dh[3][1], it["cost"][0], it["cost"][1], rows, wp, 9, 128, cv, grads[0], cin_dst=0, cin_valid=D,
                      accumulate=i > 0)
        # first layer, x_d3 channels: ONE weight gradient with sum_i dh1_i (the x_d3 part is the same in every iteration)
        lib.wgrad(acc_planes[0], acc_planes[1], gin_hi[:, Dp:], gin_lo[:, Dp:], rows, wp, 9, 128, 256, grads[0], cin_dst=D,
                  grad_b=grads[1])
        return grads


class _HeadsTrainHIP(torch.autograd.Function):
    """Outputs: the upsampled predictions of every iteration.  Inputs: the 16 trainable tensors of g_net / mask_head, so that
    autograd accumulates the gradients into their ordinary .grad."""

    @staticmethod
    def forward(ctx, runner, *params):
        outs = runner.forward()
        ctx.runner = runner
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_ups):
        grads = ctx.runner.backward(grad_ups)
        ctx.runner = None
        return (None, *grads)


def refine_train_hip(model, matcher, ref_gmms, x_d3, n_iter):
    """MAGNET.py:146-175 under autograd with g_net / mask_head on the HIP training path.  Returns the list of (B,2,4h,4w)."""
    if n_iter == 0:
        return []
    if model.downsample_ratio != 4 or x_d3.shape[1] != 256:
        raise lib.MagnetError("train_backend='hip' needs downsample_ratio 4 and a 256-channel x_d3 (the reference's heads)")
    for net in (model.g_net.gnet, model.mask_head):
        ConvStackMFMA(net)                                  # validates the stack structure (raises MagnetError otherwise)
    runner = _Runner(model, matcher, ref_gmms, x_d3, n_iter)
    return list(_HeadsTrainHIP.apply(runner, *_params(model)))
