"""Depth metrics and logging with the reference's names and formats (utils/utils.py:106-197), with the per-pixel
reductions on the device (magnet_depth_metrics) so the (B,2,H,W) predictions are never copied to the host —
the reference's validate() does `.cpu().numpy()` on full maps (test_MaGNet.py:54-56)."""
from __future__ import annotations

import ctypes
import math

import torch

from . import lib

METRIC_ORDER = ("abs_rel", "abs_diff", "sq_rel", "rmse", "rmse_log", "irmse", "log_10", "silog", "a1", "a2", "a3", "nll")


def crop_window(kind, H: int, W: int):
    """Evaluation window (y0, y1, x0, x1) of the reference's KITTI crops (test_MaGNet.py:63-71): 'garg' (Garg ECCV16),
    'eigen' (Eigen NIPS14) or None (whole frame)."""
    if kind in (None, "", "none"):
        return None
    if kind == "garg":
        return int(0.40810811 * H), int(0.99189189 * H), int(0.03594771 * W), int(0.96405229 * W)
    if kind == "eigen":
        return int(0.3324324 * H), int(0.91351351 * H), int(0.0359477 * W), int(0.96405229 * W)
    raise ValueError(f"unknown crop {kind!r}")


def depth_metric_sums(pred: torch.Tensor, gt: torch.Tensor, min_depth: float, max_depth: float, crop=None) -> torch.Tensor:
    """pred (B,2,H,W) fp32 [mu, sigma]; gt (B,1,H,W) or (B,H,W) fp32 -> (B,16) float64 sums (device).
    crop: None, 'garg', 'eigen' or an explicit (y0, y1, x0, x1) window.  Fixed summation order: deterministic."""
    p = lib._dev(pred.detach().float().contiguous(), "pred", torch.float32)
    g = lib._dev(gt.detach().float().contiguous(), "gt", torch.float32)
    B, two, H, W = p.shape
    if two != 2 or g.numel() != B * H * W:
        raise lib.MagnetError(f"depth_metric_sums: pred {tuple(p.shape)} / gt {tuple(g.shape)} mismatch")
    sums = torch.empty((B, 16), dtype=torch.float64, device=p.device)
    win = crop_window(crop, H, W) if isinstance(crop, (str, type(None))) else tuple(int(c) for c in crop)
    if win is None:
        lib._launch("magnet_depth_metrics", p, p.data_ptr(), g.data_ptr(), sums.data_ptr(), B, H * W, float(min_depth), float(max_depth))
    else:
        lib._launch("magnet_depth_metrics_crop", p, p.data_ptr(), g.data_ptr(), sums.data_ptr(), B, H, W, float(min_depth),
                    float(max_depth), *win)
    return sums


def metrics_from_sums(s) -> dict:
    """One frame's 16 sums -> the reference's metric dict (same keys as utils.compute_depth_errors)."""
    s = [float(x) for x in s]
    n = s[0]
    if n <= 0:
        return {k: float("nan") for k in METRIC_ORDER}
    mean_err = s[6] / n
    return dict(a1=s[9] / n, a2=s[10] / n, a3=s[11] / n, abs_diff=s[1] / n, abs_rel=s[2] / n, sq_rel=s[3] / n,
                rmse=math.sqrt(s[4] / n), log_10=s[7] / n, irmse=math.sqrt(s[8] / n), rmse_log=math.sqrt(s[5] / n),
                silog=math.sqrt(max(s[5] / n - mean_err * mean_err, 0.0)) * 100, nll=s[12] / n)


def compute_depth_errors(pred, gt, min_depth, max_depth, crop=None) -> list:
    """Per-frame metric dicts for a batch (device reductions, one small D2H of B x 16 doubles); crop: see depth_metric_sums."""
    return [metrics_from_sums(row) for row in depth_metric_sums(pred, gt, min_depth, max_depth, crop).cpu().tolist()]


_KINDS = {"sigma": lib.METRICS_SIGMA, "variance": lib.METRICS_VARIANCE, None: lib.METRICS_NONE}


class MetricTable:
    """The per-frame metric rows of one evaluation, kept on the device: append() launches magnet_depth_metrics_ex with `rows`
    pointing at the next free row and advances a host-side cursor (the host knows B), so the host never waits for a batch —
    rows() is read once, at the end.  kind: what the second plane holds, 'sigma' (MAGNET: squared, then clamped), 'variance' (the
    stand-alone D-Net: clamped as it is, utils.py:133) or None (the F-Net: no uncertainty, nll 0.0).  crop: None, 'garg', 'eigen'
    or a (y0, y1, x0, x1) window.  All launches go to the current stream of `device`; a full table doubles (a device copy)."""

    def __init__(self, device, min_depth: float, max_depth: float, crop=None, kind="sigma", capacity: int = 256):
        if kind not in _KINDS:
            raise ValueError(f"unknown kind {kind!r} ('sigma', 'variance' or None)")
        if capacity <= 0:
            raise ValueError("capacity must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise lib.MagnetError(f"MetricTable on {self.device}; magnet_amd runs on the GPU only (no CPU fallback)")
        self.min_depth, self.max_depth, self.crop, self.kind = float(min_depth), float(max_depth), crop, kind
        self._rows = torch.empty((int(capacity), len(METRIC_ORDER)), dtype=torch.float64, device=self.device)
        self._n = 0
        self._work = {}                                        # B -> scratch of magnet_depth_metrics_workspace(B) bytes

    def __len__(self):
        return self._n

    def rows(self) -> torch.Tensor:
        """Device (n, 12) float64 view of what has been appended, columns in METRIC_ORDER."""
        return self._rows[:self._n]

    def _plane(self, t, name, B=None, H=None, W=None):
        """(B,H,W) or (B,1,H,W) fp32 with contiguous planes -> (tensor, batch stride in elements)."""
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.device != self.device:
            raise lib.MagnetError(f"{name} must be an fp32 tensor on {self.device} (no CPU fallback)")
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        if t.dim() != 3 or (B is not None and tuple(t.shape) != (B, H, W)):
            raise lib.MagnetError(f"{name} has shape {tuple(t.shape)}, expected (B,H,W) or (B,1,H,W)" + ("" if B is None else f" = ({B},{H},{W})"))
        if not ((t.shape[2] == 1 or t.stride(2) == 1) and (t.shape[1] == 1 or t.stride(1) == t.shape[2])):
            raise lib.MagnetError(f"{name}: every H x W plane must be contiguous (strides {t.stride()})")
        return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2])

    def append(self, mu, gt, second=None):
        """mu, second: (B,H,W) or (B,1,H,W) fp32 planes (any batch stride); gt (B,1,H,W) or (B,H,W).  Nothing is read back."""
        mu, mu_stride = self._plane(mu, "mu")
        B, H, W = mu.shape
        gt, _ = self._plane(gt.detach() if isinstance(gt, torch.Tensor) else gt, "gt", B, H, W)
        gt = gt.contiguous()
        if (second is None) != (self.kind is None):
            raise lib.MagnetError(f"kind={self.kind!r} takes {'no' if self.kind is None else 'a'} second plane")
        if self._n + B > self._rows.shape[0]:
            grown = torch.empty((max(2 * self._rows.shape[0], self._n + B), self._rows.shape[1]), dtype=torch.float64, device=self.device)
            grown[:self._n].copy_(self._rows[:self._n])
            self._rows = grown
        work = self._work.get(B)
        if work is None:
            nbytes = int(lib.load().magnet_depth_metrics_workspace(B))
            if nbytes < 0:
                lib._check(-nbytes, "magnet_depth_metrics_workspace")
            work = self._work[B] = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
        a = lib.MagnetDepthMetricsArgs()
        a.mu, a.mu_stride, a.gt = mu.data_ptr(), mu_stride, gt.data_ptr()
        if second is not None:
            second, a.second_stride = self._plane(second, "second", B, H, W)
            a.second = second.data_ptr()
        a.B, a.H, a.W, a.kind = B, H, W, _KINDS[self.kind]
        a.min_depth, a.max_depth = self.min_depth, self.max_depth
        win = crop_window(self.crop, H, W) if isinstance(self.crop, (str, type(None))) else tuple(int(c) for c in self.crop)
        if win is not None:
            a.crop, (a.y0, a.y1, a.x0, a.x1) = 1, win
        a.rows = self._rows.data_ptr() + self._n * self._rows.shape[1] * 8
        a.work = work.data_ptr()
        lib._launch("magnet_depth_metrics_ex", self.device, ctypes.byref(a))
        self._n += B

    def append_pred(self, pred, gt):
        """pred (B,2,H,W) fp32: channel 0 = mu, channel 1 = the second plane, addressed through the tensor's strides (no copy)."""
        if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or pred.shape[1] != 2:
            raise lib.MagnetError("append_pred: pred must be (B,2,H,W)")
        pred = pred.detach()
        self.append(pred[:, 0], gt, None if self.kind is None else pred[:, 1])


class RunningAverage:
    def __init__(self):
        self.avg = 0
        self.count = 0

    def append(self, value):
        self.avg = (value + self.count * self.avg) / (self.count + 1)
        self.count += 1

    def get_value(self):
        return self.avg


class RunningAverageDict:
    """utils.RunningAverageDict (utils/utils.py:160-174)."""

    def __init__(self):
        self._dict = None

    def update(self, new_dict):
        if self._dict is None:
            self._dict = {key: RunningAverage() for key in new_dict}
        for key, value in new_dict.items():
            self._dict[key].append(value)

    def get_value(self):
        return {key: value.get_value() for key, value in self._dict.items()}


def format_metrics(metrics) -> str:
    return "%.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f" % tuple(metrics[k] for k in METRIC_ORDER)


def log_metrics(txt_path, metrics, first_line):
    """utils.log_metrics (utils/utils.py:177-197): same header, same 12-column line, appended to txt_path."""
    header = "abs_rel abs_diff sq_rel rmse rmse_log irmse log_10 silog a1 a2 a3 NLL"
    print("{}".format(first_line)); print(header); print(format_metrics(metrics))
    if txt_path:
        with open(txt_path, "a") as f:
            f.write("{}\n".format(first_line)); f.write(header + "\n"); f.write(format_metrics(metrics) + "\n\n")
