"""Host-side pieces that every runner of the matrix-core convolutions shares (convnet.py, fnet.py, dnet.py, train_fnet.py, train.py):
split-bf16 planes and their allocator, the weight packers, the cache that repacks when a tensor changed, and the event bracket."""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn


def round_up(x, m):
    return (x + m - 1) // m * m


def split_bf16(x: torch.Tensor):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


def planes(rows, c, dev, zero=False):
    """A (hi, lo) pair of bf16 planes (rows, c).  zero: for grids whose border (or padding channels) is read and never written."""
    new = torch.zeros if zero else torch.empty
    return new((rows, c), dtype=torch.bfloat16, device=dev), new((rows, c), dtype=torch.bfloat16, device=dev)


def plane_f16(rows, c, dev, zero=False):
    """ONE fp16 plane (rows, c): an activation buffer of the single-plane fp16 format (FNetMFMA(precision="fp16"))."""
    return (torch.zeros if zero else torch.empty)((rows, c), dtype=torch.float16, device=dev)


def fold_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    """Conv2d (with or without bias) followed by eval-mode BatchNorm2d -> (weight, bias) in fp64: w * s, (b - mean) * s + beta,
    s = gamma / sqrt(var + eps)."""
    w = conv.weight.detach().double()
    b = conv.bias.detach().double() if conv.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return w * s.view(-1, 1, 1, 1), (b - bn.running_mean.detach().double()) * s + bn.bias.detach().double()


def pack_taps(w: torch.Tensor, cin_pad=None):
    """(cout, cin, kh, kw) -> split bf16 planes (kh*kw, cout, cin_pad or cin), cin contiguous, the padding channels zero."""
    cout, cin, kh, kw = w.shape
    wt = w.float().permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
    if cin_pad is not None and cin_pad != cin:
        wt = torch.cat([wt, wt.new_zeros((kh * kw, cout, cin_pad - cin))], dim=2)
    return split_bf16(wt.contiguous())


def to_f16_sat(x: torch.Tensor):
    """fp32 -> fp16 as the single-plane fp16 format defines it (include/magnet_hip.h): round to nearest even, magnitudes that would
    round above 65504 (+-Inf included) become +-65504, NaN stays NaN, the sign of zero is kept."""
    return x.float().clamp(-65504.0, 65504.0).to(torch.float16)


def pack_taps_f16(w: torch.Tensor, cin_pad=None):
    """(cout, cin, kh, kw) fp32 -> ONE fp16 plane (kh*kw, cout, cin_pad or cin), cin contiguous, the padding channels zero: the weight
    operand of lib.conv_mfma(f16=True)."""
    cout, cin, kh, kw = w.shape
    wt = w.float().permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
    if cin_pad is not None and cin_pad != cin:
        wt = torch.cat([wt, wt.new_zeros((kh * kw, cout, cin_pad - cin))], dim=2)
    return to_f16_sat(wt).contiguous()


def s2d_matrix(w: torch.Tensor):
    """3x3 stride-2 pad-1 weights (cout, C, 3, 3) -> the equivalent 2x2-window weights over a space-to-depth input: fp32
    (4, cout, 4*C); tap (ty,tx) in {-1,0}^2 -> index (ty+1)*2+(tx+1); channel (py*2+px)*C + c."""
    cout, C = w.shape[:2]
    out = torch.zeros((4, cout, 4 * C), dtype=torch.float32, device=w.device)
    k_of = {(-1, 1): 0, (0, 0): 1, (0, 1): 2}                       # (tap offset, phase) -> kernel index; (-1, 0) has none
    for (ty, py), ky in k_of.items():
        for (tx, px), kx in k_of.items():
            ph = py * 2 + px
            out[(ty + 1) * 2 + (tx + 1), :, ph * C:(ph + 1) * C] = w[:, :, ky, kx]
    return out


def pack_s2d(w: torch.Tensor):
    return split_bf16(s2d_matrix(w))


def pack_s2d_f16(w: torch.Tensor):
    """pack_s2d on the single-plane fp16 format: ONE fp16 plane (4, cout, 4*C), each weight rounded once (to_f16_sat)."""
    return to_f16_sat(s2d_matrix(w)).contiguous()


class PackCache:
    """What a runner derives from its module's tensors, rebuilt when one of them changed.  The rule: a value is valid for the key
    ((data_ptr, _version) of every tensor) + (str(device),).  An optimizer step, load_state_dict or a BatchNorm update writes in place
    and bumps _version; a replaced tensor has another data_ptr.  `tensors`: a callable returning the tensors to watch."""

    def __init__(self, tensors):
        self._tensors = tensors
        self._key = None
        self._vals = {}

    def get(self, device, build, *entry):
        """The value stored under `entry` for the tensors as they are now on `device`, or build() (stored)."""
        key = tuple((t.data_ptr(), t._version) for t in self._tensors()) + (str(device),)
        if key != self._key:
            self._key = key
            self._vals = {}
        if entry not in self._vals:
            self._vals[entry] = build()
        return self._vals[entry]


@contextlib.contextmanager
def _bracket(sink, payload):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    yield
    e1.record()
    sink.append((e0, e1) + payload)


_UNTIMED = contextlib.nullcontext()


def timed(sink, *payload):
    """`with timed(sink, ...): <one launch>` records a timing event before and after the launch on the current stream and appends
    (start, end, *payload) to the list `sink`; with sink None it is one shared do-nothing context."""
    return _UNTIMED if sink is None else _bracket(sink, payload)
