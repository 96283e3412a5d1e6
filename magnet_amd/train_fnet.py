"""The F-Net's forward in training mode on HIP (MAGNET_F(..., train_backend="hip"); reference train_FNet.py:69-119, which runs
the F-Net under model.train()).

Every convolution runs on the inference kernel (lib.conv_mfma, bf16x3 on the matrix cores) with the module's own weights, no
BatchNorm folding, no bias, and an fp32 pre-BN output; firstconv.0 runs on magnet_fnet_stem_raw.  Each BatchNorm2d then takes
the statistics of the whole batch (all B(1+V) images of MAGNET_F's single f_net call, as torch does) with a deterministic
fp64 two-stage reduction and updates running_mean, running_var (unbiased, the module's momentum) and num_batches_tracked on the
device, once per forward (csrc/train_fnet_fwd.hip).  The same kernel applies the affine, the BasicBlock's residual (the input,
or bn(downsample(x))) and the ReLU, and writes the next layer's zero-bordered split-bf16 planes, the 320-channel concatenation
slices included.  The SPP branches take their statistics over the pooled grids (N cells for branch1 at H/4 = 64).

Backward (_FNetTrainFn, an autograd.Function that takes every F-Net parameter as an input, so .grad accumulates normally): the
feature gradient enters the bordered split-bf16 grid (magnet_fnet_grad_pack); per layer, in reverse order, BatchNorm backward with
the ReLU mask (magnet_bn_train_backward), the weight gradient on the matrix cores (magnet_wgrad_ex: dilation 2, border 2, the
space-to-depth window, cin up to 320), and the input gradient on conv_mfma with flipped, transposed weight packs.  The stride-2
layers take the mirrored 2x2 window by reading the gradient one row and one column further (an input offset of wp + 1 rows), then
magnet_fnet_d2s_backward.  Gradient fan-in (unit input = conv1 + shortcut, raw = concat + layer3, skip = concat + four SPP branches)
is summed in a fixed order, in the convolution epilogue (addend) or in magnet_spp_pool_backward.  The stem's weight gradient is
magnet_fnet_stem_wgrad.  Every sum has a fixed order and no atomics: two identical steps give bit-identical .grad.

Synchronised BatchNorm (the reference's multi-GPU pattern, train_FNet.py:220-222: nn.SyncBatchNorm.convert_sync_batchnorm, then
DistributedDataParallel): a slot that holds an nn.SyncBatchNorm in training mode, with torch.distributed initialised and more than
one rank in the module's process group (sync_group), takes its statistics over all ranks' shards.  Forward: the rank's fp64
(n, mean, M2) record per channel (magnet_bn_sync_moments), one all-gather on the module's group, the records merged in rank order
(magnet_bn_sync_merge: every rank does the same arithmetic on the same bytes, so mean, invstd and the running statistics are
bit-identical across ranks), then the same apply.  Backward: the rank's sums of g' and g' xhat (magnet_bn_sync_backward_sums), one
all-gather, the sums added in rank order and dx (magnet_bn_sync_backward_apply).  dgamma / dbeta stay the rank's own sums, as
torch.nn.SyncBatchNorm leaves them: DDP averages parameter gradients.  Ranks may hold different numbers of images (H, W agree);
a rank needs one pooled cell, not two.  Every other case (BatchNorm2d, no process group, one rank, .eval()) runs the launches
above unchanged.

Memory kept for the backward per image (P2 = (H/2+2)(W/2+2), P4 = (H/4+4)(W/4+4) grid rows): every layer's fp32 pre-BN output
and split-bf16 output, P2 x 8 layers x 32 ch x 8 B + P4 x (34 x 64 + 12 x 128 + 128 + 320 + 128) ch x 8 B: about 0.9 GB at
480 x 640.  Under no_grad nothing is kept.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn as nn

from . import lib
from .fnet import _SPP, convs
from .planes import PackCache, pack_s2d, pack_taps, planes, s2d_matrix, split_bf16


def sync_group(bn: nn.Module):
    """The process group over which the BatchNorm slot `bn` synchronises its statistics, or None for the single-process launches:
    an nn.SyncBatchNorm in training mode, torch.distributed initialised, and more than one rank in the module's process_group
    (None: the default group) - the conditions under which torch's own SyncBatchNorm synchronises."""
    if not isinstance(bn, nn.SyncBatchNorm) or not bn.training:
        return None
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) > 1 else None


def bn_merge_records(records):
    """The merge of magnet_bn_sync_merge in Python floats (fp64), in rank order: records = [(n_r, mean_r, M2_r), ...] of one channel,
    M2_r = sum (x - mean_r)^2 over the shard -> (n_tot, mean, M2) of the concatenated data (Chan et al.'s pairwise update, stated
    for all ranks at once): n_tot = sum n_r, mean = sum n_r mean_r / n_tot, M2 = sum (M2_r + n_r (mean_r - mean)^2)."""
    n_tot, s = 0.0, 0.0
    for n, mean, _ in records:
        n_tot += n
        s += n * mean
    mean_tot = s / n_tot
    M2 = 0.0
    for n, mean, m2 in records:
        d = mean - mean_tot
        M2 += m2 + n * (d * d)
    return n_tot, mean_tot, M2


def check_input(img: torch.Tensor, psm: nn.Module, sync: bool = False):
    """The shapes the training forward supports (those FNetMFMA accepts): raises MagnetError before any launch.  sync: the
    statistics are taken over several ranks (sync_group), so one pooled cell on this rank is enough."""
    if img.dim() != 4 or img.shape[1] != 3:
        raise lib.MagnetError(f"F-Net training forward: image batch must be (N, 3, H, W), got {tuple(img.shape)}")
    N, _, H, W = img.shape
    H4, W4 = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    if H4 < 64 or W4 < 64:
        raise lib.MagnetError(f"F-Net training forward: input {H}x{W} too small for the 64x64 pooling branch (needs H/4, W/4 >= 64)")
    if N * (H4 // 64) * (W4 // 64) < (1 if sync else 2):
        raise lib.MagnetError("F-Net training forward: BatchNorm with batch statistics needs at least 2 values per channel, and "
                              f"branch1 pools {N} image(s) of {H}x{W} to {N * (H4 // 64) * (W4 // 64)} cell(s)")
    fd = psm.lastconv[2].weight.shape[0]
    if fd not in (16, 32, 64, 128):
        raise lib.MagnetError(f"F-Net training forward: feature_dim {fd} unsupported (16, 32, 64, 128)")
    for m in psm.modules():
        if isinstance(m, (nn.BatchNorm2d, nn.SyncBatchNorm)) and not m.affine:
            raise lib.MagnetError("F-Net training forward: BatchNorm2d without affine parameters is not supported")
    if not img.is_cuda:
        raise lib.MagnetError("F-Net training forward: image must be on the GPU (no CPU fallback)")


def bn_running_update(running_mean, running_var, mean, var_biased, n, momentum, num_batches_tracked):
    """nn.BatchNorm2d's running-statistics update in training mode, as magnet_bn_train_stats computes it (in fp64):
    m = momentum, or 1 / (num_batches_tracked + 1) when momentum is None; running = (1 - m) running + m stat, the variance
    unbiased (n / (n - 1)).  Returns (running_mean, running_var, num_batches_tracked + 1)."""
    m = (1.0 / (num_batches_tracked + 1)) if momentum is None else momentum
    return ((1.0 - m) * running_mean + m * mean, (1.0 - m) * running_var + m * var_biased * n / (n - 1.0), num_batches_tracked + 1)


def s2d_grad_to_3x3(g4: torch.Tensor, C: int):
    """Weight gradient over the space-to-depth 2x2 window (cout, 4C, 2, 2) -> the 3x3 stride-2 layer's (cout, C, 3, 3): every 3x3
    tap is exactly one (window tap, phase) pair."""
    out = torch.empty((g4.shape[0], C, 3, 3), dtype=g4.dtype, device=g4.device)
    k_of = {(-1, 1): 0, (0, 0): 1, (0, 1): 2}
    for (ty, py), ky in k_of.items():
        for (tx, px), kx in k_of.items():
            ph = py * 2 + px
            out[:, :, ky, kx] = g4[:, ph * C:(ph + 1) * C, ty + 1, tx + 1]
    return out


def dgrad_pack(w: torch.Tensor):
    """Input-gradient weights of a stride-1 conv (cout, cin, k, k): flipped taps, transposed -> split planes (k*k, cin, cout)."""
    return pack_taps(w.flip(2, 3).transpose(0, 1).contiguous())


def dgrad_pack_s2d(w: torch.Tensor):
    """Input-gradient weights of the space-to-depth 2x2 window: tap t takes the window's tap 3 - t, transposed -> (4, 4C, cout).
    Run over the gradient read wp + 1 rows further, the window's offsets (-wp-1, -wp, -1, 0) become (0, 1, wp, wp+1): the mirror."""
    return split_bf16(s2d_matrix(w).flip(0).transpose(1, 2).contiguous())


def _all_gather(t: torch.Tensor, group):
    """(world, *t.shape): t of every rank of `group`, in rank order, on every rank.  One collective; gloo has no
    all_gather_into_tensor, so there the ranks' slices of the one output buffer go as a tensor list (as torch's SyncBatchNorm does)."""
    out = torch.empty((dist.get_world_size(group),) + tuple(t.shape), dtype=t.dtype, device=t.device)
    if dist.get_backend(group) == "gloo":
        dist.all_gather(list(out.unbind(0)), t, group=group)
    else:
        dist.all_gather_into_tensor(out, t, group=group)
    return out


class FNetTrainHIP:
    """Training-mode forward (and, after a forward with save=True, backward) runner for a `PSMNet` (or the reference's own PSMNet
    instance: same attribute structure)."""

    def __init__(self, psm: nn.Module):
        self.psm = psm
        self._packed = None
        self._cache = PackCache(lambda: list(psm.parameters()))
        self._work = {}
        self.rec = None

    def packed(self, device):
        """The module's conv weights as split-bf16 tap planes (no folding), with a zero bias; repacked when a weight changes."""
        self._packed = self._cache.get(device, lambda: self._pack(device))
        return self._packed

    @torch.no_grad()
    def _pack(self, device):
        P = {}
        for name, conv, _, s2d in convs(self.psm):
            w = conv.weight.detach().float().to(device)
            if name == "firstconv.0":
                P["stem"] = w.reshape(32, 27).contiguous()
            else:
                P[name] = (*(pack_s2d if s2d else pack_taps)(w), torch.zeros(w.shape[0], dtype=torch.float32, device=device), w.shape[0])
        return P

    def _ws(self, dev, n):
        w = self._work.get(str(dev))
        if w is None or w.numel() < n:
            w = self._work[str(dev)] = torch.empty(n, dtype=torch.float64, device=dev)
        return w

    def _bn(self, name, z, grid, relu, out=None, out_f32=None, res=None):
        bn = self._bn_mods[name]
        C = grid[-1]
        stats = torch.empty(2, C, dtype=torch.float32, device=z.device)
        work = self._ws(z.device, lib.BN_BLOCKS * 320 * 2)
        group = sync_group(bn)
        sync = {}
        if group is not None:
            # the rank's record -> every rank's records, in rank order -> the global statistics; the apply below is the same launch
            record = torch.empty(3, C, dtype=torch.float64, device=z.device)
            lib.bn_sync_moments(z, grid, work, record)
            n_tot = torch.empty(1, dtype=torch.float64, device=z.device)
            lib.bn_sync_merge(_all_gather(record, group), C, stats[0], stats[1], n_tot, bn.eps, bn.momentum, running_mean=bn.running_mean,
                              running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked)
            sync = dict(n_tot=n_tot, group=group)
        lib.bn_train(z, grid, stats[0], stats[1], work, bn.weight.detach(), bn.bias.detach(),
                     bn.eps, bn.momentum, running_mean=bn.running_mean, running_var=bn.running_var,
                     num_batches_tracked=bn.num_batches_tracked, res=res, relu=relu, out=out, out_f32=out_f32, stats=group is None)
        if self.rec is not None:
            self.rec[name].update(z=z, stats=stats, grid=grid, relu=relu, **sync)

    def _layer(self, name, src, in_ld, cin, taps, wp, rows, grid, relu, dst, res=None, dil=0):
        hi, lo, zb, cout = self._packed[name]
        z = torch.empty((rows, cout), dtype=torch.float32, device=src[0].device)
        lib.conv_mfma(src[0], src[1], in_ld, cin, hi, lo, zb, taps, wp, False, rows, out_f32=z, dil=dil)
        if self.rec is not None:
            self.rec[name] = dict(x=src, out=dst, taps=taps, dil=dil, cin=cin, wp=wp, rows=rows)
        self._bn(name, z, grid + (cout,), relu, out=dst, res=res)

    @torch.no_grad()
    def run(self, img: torch.Tensor, save: bool = False) -> torch.Tensor:
        """img (N,3,H,W) fp32 on the GPU -> the (N,F,H/4,W/4) fp32 NCHW features of the module in training mode; every
        BatchNorm2d's running statistics and num_batches_tracked are updated once.  save: keep what backward() needs."""
        psm = self.psm
        check_input(img, psm, sync=sync_group(psm.branch1[1][1]) is not None)  # branch1 pools to the fewest cells
        img = img.detach().float().contiguous()
        N, _, H, W = img.shape
        dev = img.device
        for t in list(psm.parameters()) + [b for b in psm.buffers() if b is not None]:
            if t.device != dev:
                raise lib.MagnetError(f"F-Net training forward: module tensors must be on {dev}")
        P = self.packed(dev)
        self._bn_mods = {name: bn for name, _, bn, _ in convs(psm) if bn is not None}     # in forward order
        self.rec = {} if save else None
        H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
        rows_a, rows_b = N * (H2 + 2) * (W2 + 2), N * (H4 + 4) * (W4 + 4)
        wpa, wpb = W2 + 2, W4 + 4
        ga, gb = (N, H2 + 2, wpa, 1), (N, H4 + 4, wpb, 2)
        self.dims = (N, H, W, H2, W2, H4, W4, rows_a, rows_b)
        self.img = img

        # ---- H/2 stage: firstconv + layer1 (32 channels, border 1) ----
        z = torch.empty((rows_a, 32), dtype=torch.float32, device=dev)
        lib.fnet_stem_raw(img, P["stem"], z)                                                     # F_psmnet.py:40
        a0 = planes(rows_a, 32, dev)
        if save:
            self.rec["firstconv.0"] = dict(out=a0)
        self._bn("firstconv.0", z, ga + (32,), True, out=a0)
        a1 = planes(rows_a, 32, dev)
        self._layer("firstconv.2", a0, 32, 32, 9, wpa, rows_a, ga, True, a1)
        x = planes(rows_a, 32, dev)
        self._layer("firstconv.4", a1, 32, 32, 9, wpa, rows_a, ga, True, x)
        for i in range(3):                                                                       # layer1
            t, o = planes(rows_a, 32, dev), planes(rows_a, 32, dev)
            self._layer(f"layer1.{i}.conv1", x, 32, 32, 9, wpa, rows_a, ga, True, t)
            self._layer(f"layer1.{i}.conv2", t, 32, 32, 9, wpa, rows_a, ga, False, o, res=x)
            x = o
        # ---- H/4 stage (border 2: layer4 is dilated) ----
        S = planes(rows_b, 128, dev, zero=True)
        lib.space_to_depth(x[0], x[1], S[0], S[1], N, 32, H2, W2, 2)
        b0, b1, b2 = planes(rows_b, 64, dev), planes(rows_b, 64, dev), planes(rows_b, 64, dev)
        self._layer("layer2.0.conv1", S, 128, 128, 4, wpb, rows_b, gb, True, b0)                # 3x3 stride 2
        self._layer("layer2.0.downsample", (S[0][:, :32], S[1][:, :32]), 128, 32, 1, wpb, rows_b, gb, False, b1)   # phase 0
        self._layer("layer2.0.conv2", b0, 64, 64, 9, wpb, rows_b, gb, False, b2, res=b1)
        cur, ld = b2, 64
        cat = planes(rows_b, 320, dev, zero=True)
        raw = (cat[0][:, 0:64], cat[1][:, 0:64])
        for i in range(1, 16):
            t = planes(rows_b, 64, dev)
            self._layer(f"layer2.{i}.conv1", cur, ld, 64, 9, wpb, rows_b, gb, True, t)
            last = i == 15                                                                       # output_raw -> concat[:, 0:64]
            o = raw if last else planes(rows_b, 64, dev)
            self._layer(f"layer2.{i}.conv2", t, 64, 64, 9, wpb, rows_b, gb, False, o, res=cur)
            cur, ld = (raw, 320) if last else (o, 64)
        skip = (cat[0][:, 64:192], cat[1][:, 64:192])
        units = [("layer3", i, 0) for i in range(3)] + [("layer4", i, 2) for i in range(3)]
        for n_unit, (name, i, dil) in enumerate(units):
            cin = 64 if (name == "layer3" and i == 0) else 128
            t = planes(rows_b, 128, dev)
            self._layer(f"{name}.{i}.conv1", cur, ld, cin, 9, wpb, rows_b, gb, True, t, dil=dil)
            if f"{name}.{i}.downsample" in P:
                r = planes(rows_b, 128, dev)
                self._layer(f"{name}.{i}.downsample", cur, ld, cin, 1, wpb, rows_b, gb, False, r)
                res = r
            else:
                res = cur
            last = n_unit == len(units) - 1                                                      # output_skip -> concat[:, 64:192]
            o = skip if last else planes(rows_b, 128, dev)
            self._layer(f"{name}.{i}.conv2", t, 128, 128, 9, wpb, rows_b, gb, False, o, res=res, dil=dil)
            cur, ld = (skip, 320) if last else (o, 128)
        # ---- SPP branches: pool -> 1x1 conv -> BN over the pooled cells -> ReLU -> bilinear back to H/4 into the concat ----
        for slot, (name, k) in enumerate(_SPP):                     # branch1 -> channels 288:320 ... branch4 -> 192:224
            ph, pw = H4 // k, W4 // k
            cells = N * ph * pw
            pool = planes(cells, 128, dev)
            lib.avgpool_cl(skip[0], skip[1], 320, N, H4, W4, 2, k, 128, pool[0], pool[1])
            hi, lo, zb, _ = P[name]
            zq = torch.empty((cells, 32), dtype=torch.float32, device=dev)
            q = torch.empty((cells, 32), dtype=torch.float32, device=dev)
            lib.conv_mfma(pool[0], pool[1], 128, 128, hi, lo, zb, 1, 1, False, cells, out_f32=zq)
            if save:
                self.rec[name] = dict(x=pool, k=k, ph=ph, pw=pw, off=288 - 32 * slot)
            self._bn(name, zq, (N, ph, pw, 0, 32), True, out_f32=q)
            off = 288 - 32 * slot
            lib.upsample_bilinear_cl(q, 32, ph, pw, 32, cat[0][:, off:off + 32], cat[1][:, off:off + 32], 320, N, H4, W4, 2)
        # ---- lastconv ----
        c0 = planes(rows_b, 128, dev)
        self._layer("lastconv.0", cat, 320, 320, 9, wpb, rows_b, gb, True, c0)
        Fd = P["lastconv.2"][3]
        out = torch.empty((N, H4, W4, Fd), dtype=torch.float32, device=dev)
        hi, lo, zb, _ = P["lastconv.2"]
        lib.conv_mfma(c0[0], c0[1], 128, 128, hi, lo, zb, 1, wpb, False, rows_b, border=(H4 + 4, 2), repad=1, out_f32=out, out_ld=Fd)
        if save:
            self.rec["lastconv.2"] = dict(x=c0)
        # the running statistics changed on the device behind autograd's back: bump their version counters, so that caches keyed
        # on them (FNetMFMA's folded weights) see the change
        for bn in self._bn_mods.values():
            for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
                if t is not None:
                    torch.autograd.graph.increment_version(t)
        return out.permute(0, 3, 1, 2).contiguous()

    # ---- backward ------------------------------------------------------------------------------------------------------
    def _bn_bwd(self, name, g):
        """BatchNorm backward of layer `name` for the output gradient g (fp32 grid): dz split planes; dgamma / dbeta recorded."""
        r, bn = self.rec[name], self._bn_mods[name]
        grid = r["grid"]
        rows = grid[0] * grid[1] * grid[2]
        dz = planes(rows, grid[4], g.device)
        dgamma = torch.empty_like(bn.weight, dtype=torch.float32)
        dbeta = torch.empty_like(bn.bias, dtype=torch.float32)
        work = self._ws(g.device, (lib.BN_BLOCKS * 2 + 2) * 320)
        bn_args = (r["z"], grid, r["stats"][0], r["stats"][1], bn.weight.detach(), bn.bias.detach(), r["relu"], g)
        if "group" in r:                                            # the forward synchronised: so does the backward
            sums = torch.empty(2, grid[4], dtype=torch.float64, device=g.device)
            lib.bn_sync_backward_sums(*bn_args, dgamma, dbeta, work, sums)
            lib.bn_sync_backward_apply(*bn_args, dz, work, _all_gather(sums, r["group"]), r["n_tot"])
        else:
            lib.bn_train_backward(*bn_args, dgamma, dbeta, dz, work)
        self.grads[id(bn.weight)], self.grads[id(bn.bias)] = dgamma, dbeta
        return dz

    def _wgrad(self, name, conv, dz):
        r = self.rec[name]
        w = conv.weight
        cout, cin_w = w.shape[:2]
        x = r["x"]
        if r["taps"] == 4:                                          # layer2.0.conv1: over the space-to-depth window
            g4 = torch.empty((cout, 4 * cin_w, 2, 2), dtype=torch.float32, device=dz[0].device)
            lib.wgrad_ex(dz[0], dz[1], x[0], x[1], r["rows"], r["wp"], 4, cout, 4 * cin_w, g4)
            gw = s2d_grad_to_3x3(g4, cin_w).contiguous()
        else:
            gw = torch.empty(w.shape, dtype=torch.float32, device=dz[0].device)
            lib.wgrad_ex(dz[0], dz[1], x[0], x[1], r["rows"], max(r["wp"], 3), r["taps"], cout, r["cin"], gw, dil=max(r["dil"], 1))
        self.grads[id(w)] = gw

    def _dgrad(self, name, conv, dz, out, addend=None):
        """Input gradient of a stride-1 convolution into the fp32 grid `out` (+ addend, in the epilogue)."""
        r = self.rec[name]
        w = conv.weight.detach().float()
        cout = w.shape[0]
        hi, lo = dgrad_pack(w)
        zb = torch.zeros(w.shape[1], dtype=torch.float32, device=w.device)
        lib.conv_mfma(dz[0], dz[1], cout, cout, hi, lo, zb, r["taps"], r["wp"], False, r["rows"], out_f32=out, dil=r["dil"], addend=addend)

    def _unit_bwd(self, name, i, g_out, extra=None):
        """Backward of one residual unit for its output gradient; returns its input's gradient (+ extra: another consumer's)."""
        u = getattr(self.psm, name)[i]
        n1, n2, nd = f"{name}.{i}.conv1", f"{name}.{i}.conv2", f"{name}.{i}.downsample"
        dev = g_out.device
        rows = self.rec[n2]["rows"]
        cout = u.conv2[0].weight.shape[0]
        dz2 = self._bn_bwd(n2, g_out)
        self._wgrad(n2, u.conv2[0], dz2)
        dh = torch.empty((rows, cout), dtype=torch.float32, device=dev)
        self._dgrad(n2, u.conv2[0], dz2, dh)
        dz1 = self._bn_bwd(n1, dh)
        self._wgrad(n1, u.conv1[0][0], dz1)
        cin = u.conv1[0][0].weight.shape[1]
        if u.downsample is None:
            short = g_out if extra is None else None
            assert extra is None
        else:
            dzd = self._bn_bwd(nd, g_out)
            self._wgrad(nd, u.downsample[0], dzd)
            if self.rec[n1]["taps"] == 4:                           # layer2.0: phase-0 channels of the space-to-depth grid
                short = torch.zeros((rows, 4 * cin), dtype=torch.float32, device=dev)
                wd = u.downsample[0].weight.detach().float()
                hi, lo = dgrad_pack(wd)
                lib.conv_mfma(dzd[0], dzd[1], cout, cout, hi, lo, torch.zeros(cin, device=dev), 1, self.rec[nd]["wp"], False, rows,
                              out_f32=short, out_ld=4 * cin)
            else:
                short = torch.empty((rows, cin), dtype=torch.float32, device=dev)
                self._dgrad(nd, u.downsample[0], dzd, short, addend=extra)
        if self.rec[n1]["taps"] == 4:
            r = self.rec[n1]
            wp = r["wp"]
            hi, lo = dgrad_pack_s2d(u.conv1[0][0].weight.detach().float())
            dS = torch.zeros((rows, 4 * cin), dtype=torch.float32, device=dev)
            lib.conv_mfma(dz1[0][wp + 1:], dz1[1][wp + 1:], cout, cout, hi, lo, torch.zeros(4 * cin, device=dev), 4, wp, False,
                          rows - wp - 1, out_f32=dS, addend=short)
            return dS
        dx = torch.empty((rows, cin), dtype=torch.float32, device=dev)
        self._dgrad(n1, u.conv1[0][0], dz1, dx, addend=short)
        return dx

    @torch.no_grad()
    def backward(self, grad_feat: torch.Tensor):
        """The gradients of every F-Net parameter (list, in psm.parameters() order) for the feature gradient (N,F,H/4,W/4)."""
        if self.rec is None:
            raise lib.MagnetError("FNetTrainHIP.backward: no saved forward (run(..., save=True) first)")
        psm = self.psm
        N, H, W, H2, W2, H4, W4, rows_a, rows_b = self.dims
        dev = grad_feat.device
        self.grads = {}
        wpb = W4 + 4
        # ---- lastconv.2 (1x1, no BN): the feature gradient enters the bordered grid ----
        w2 = psm.lastconv[2].weight
        Fd = w2.shape[0]
        Fp = max(Fd, 32)
        dF = planes(rows_b, Fp, dev)
        lib.fnet_grad_pack(grad_feat.float().contiguous(), dF[0], dF[1], 2)
        gw = torch.empty(w2.shape, dtype=torch.float32, device=dev)
        c0 = self.rec["lastconv.2"]["x"]
        lib.wgrad_ex(dF[0], dF[1], c0[0], c0[1], rows_b, wpb, 1, Fp, 128, gw, cout_valid=Fd)
        self.grads[id(w2)] = gw
        wt = torch.zeros((128, Fp, 1, 1), dtype=torch.float32, device=dev)
        wt[:, :Fd] = w2.detach().float().transpose(0, 1)
        hi, lo = pack_taps(wt)
        g_l0 = torch.empty((rows_b, 128), dtype=torch.float32, device=dev)
        lib.conv_mfma(dF[0], dF[1], Fp, Fp, hi, lo, torch.zeros(128, device=dev), 1, wpb, False, rows_b, out_f32=g_l0)
        # ---- lastconv.0 (3x3, 320 -> 128) ----
        conv = psm.lastconv[0][0]
        dz = self._bn_bwd("lastconv.0", g_l0)
        self._wgrad("lastconv.0", conv, dz)
        g_cat = torch.empty((rows_b, 320), dtype=torch.float32, device=dev)
        wf = conv.weight.detach().float()
        for c_lo, c_hi in ((0, 128), (128, 256), (256, 320)):
            hi, lo = dgrad_pack(wf[:, c_lo:c_hi])
            lib.conv_mfma(dz[0], dz[1], 128, 128, hi, lo, torch.zeros(c_hi - c_lo, device=dev), 9, wpb, False, rows_b,
                          out_f32=g_cat[:, c_lo:], out_ld=320)
        # ---- SPP branches, then the skip connection's gradient ----
        dpools = {}
        for name, k in _SPP:
            r = self.rec[name]
            ph, pw = r["ph"], r["pw"]
            cells = N * ph * pw
            dq = torch.empty((cells, 32), dtype=torch.float32, device=dev)
            lib.spp_upsample_backward(g_cat, r["off"], N, H4, W4, 2, ph, pw, dq)
            dzq = self._bn_bwd(name, dq)
            cv = getattr(psm, name)[1][0]
            gwb = torch.empty(cv.weight.shape, dtype=torch.float32, device=dev)
            lib.wgrad_ex(dzq[0], dzq[1], r["x"][0], r["x"][1], cells, 3, 1, 32, 128, gwb)
            self.grads[id(cv.weight)] = gwb
            hi, lo = dgrad_pack(cv.weight.detach().float())
            dp = torch.empty((cells, 128), dtype=torch.float32, device=dev)
            lib.conv_mfma(dzq[0], dzq[1], 32, 32, hi, lo, torch.zeros(128, device=dev), 1, 1, False, cells, out_f32=dp)
            dpools[k] = dp
        g = torch.zeros((rows_b, 128), dtype=torch.float32, device=dev)
        lib.spp_pool_backward(g_cat, 64, N, H4, W4, 2, [dpools[k] for k in (64, 32, 16, 8)], g)
        # ---- layer4, layer3 (layer3.0's input is raw, which also feeds the concat) ----
        for name, i in [("layer4", 2), ("layer4", 1), ("layer4", 0), ("layer3", 2), ("layer3", 1)]:
            g = self._unit_bwd(name, i, g)
        g = self._unit_bwd("layer3", 0, g, extra=g_cat)             # + concat[:, 0:64] (addend_ld 320)
        for i in range(15, -1, -1):
            g = self._unit_bwd("layer2", i, g)
        # ---- space-to-depth backward, layer1, firstconv ----
        gA = torch.zeros((rows_a, 32), dtype=torch.float32, device=dev)
        lib.fnet_d2s_backward(g, gA, N, 32, H2, W2, 2)
        g = gA
        for i in range(2, -1, -1):
            g = self._unit_bwd("layer1", i, g)
        for name, idx in (("firstconv.4", 4), ("firstconv.2", 2)):
            cv = psm.firstconv[idx][0]
            dz = self._bn_bwd(name, g)
            self._wgrad(name, cv, dz)
            g = torch.empty((rows_a, 32), dtype=torch.float32, device=dev)
            self._dgrad(name, cv, dz, g)
        dz = self._bn_bwd("firstconv.0", g)
        gs = torch.empty((32, 3, 3, 3), dtype=torch.float32, device=dev)
        lib.fnet_stem_wgrad(self.img, dz, gs, self._ws(dev, lib.BN_BLOCKS * 864))
        self.grads[id(psm.firstconv[0][0].weight)] = gs
        out = [self.grads[id(p)] for p in psm.parameters()]
        self.rec, self.grads = None, None
        return out


class _FNetTrainFn(torch.autograd.Function):
    """Output: the (N,F,H/4,W/4) features in training mode.  Inputs: every F-Net parameter, so that autograd accumulates the
    gradients into their ordinary .grad (clip_grad_norm_, GradScaler and AdamW work unchanged)."""

    @staticmethod
    def forward(ctx, runner, img, *params):
        ctx.runner = runner
        return runner.run(img, save=True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_feat):
        grads = ctx.runner.backward(grad_feat.contiguous())
        ctx.runner = None
        return (None, None, *grads)


def fnet_train_hip(runner: FNetTrainHIP, img: torch.Tensor):
    """The F-Net's training-mode forward under autograd (the image takes no gradient)."""
    if img.requires_grad:
        raise lib.MagnetError("train_backend='hip': the F-Net backward gives no gradient to the input images")
    return _FNetTrainFn.apply(runner, img, *runner.psm.parameters())
