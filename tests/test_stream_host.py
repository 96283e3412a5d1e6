"""Streaming inference without a GPU (magnet_amd/sequence.py graph mode, csrc/frame_pool.hip magnet_scatter_frames): the new entry
point is declared, bound and exported, refuses bad arguments with the header's codes before any launch, its wrapper refuses CPU
tensors and wrong shapes, and SequenceRunner takes `graph` as a bool only."""
import ctypes
import os
import re

import pytest
import torch

from magnet_amd import lib
from magnet_amd.magnet import MAGNET
from magnet_amd.sequence import SequenceRunner
from magnet_amd.standin import StubDNet, StubFNet, make_args

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "magnet_hip.h")


def test_abi_grows_by_scatter_frames(hip_lib):
    assert "magnet_scatter_frames" in lib.API_SYMBOLS
    text = open(HEADER).read()
    assert re.search(r"MAGNET_API int magnet_scatter_frames\(const MagnetScatterFramesArgs \*args, void \*stream\);", text)
    assert re.search(r"#define MAGNET_HIP_VERSION 500\b", text)
    assert hasattr(hip_lib, "magnet_scatter_frames")
    assert lib.API_SYMBOLS.index("magnet_scatter_frames") == lib.API_SYMBOLS.index("magnet_gather_views") + 1


def _args(**kw):
    """A call the library accepts up to the launch: fake non-NULL, 16-byte aligned pointers everywhere."""
    a = lib.MagnetScatterFramesArgs(slots=16, n_slots=4, n=2, h=5, w=7, F=16, feat_dtype=lib.FEAT_F32, feat=32, gmm=48, xd3_hi=64, xd3_lo=80,
                                    pool_feat=96, pool_gmm=112, pool_xd3_hi=128, pool_xd3_lo=144)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_scatter_frames_argument_errors_are_codes(hip_lib):
    f = hip_lib.magnet_scatter_frames
    assert f(None, None) == lib.E_NULL
    # a NULL table, or a NULL pool tensor for a source that is given
    for kw in (dict(slots=None), dict(pool_feat=None), dict(pool_gmm=None), dict(pool_xd3_hi=None), dict(pool_xd3_lo=None)):
        assert f(ctypes.byref(_args(**kw)), None) == lib.E_NULL, kw
        assert b"magnet_scatter_frames" in hip_lib.magnet_last_error()
    # dimensions, and one x_d3 plane without the other
    for kw in (dict(F=12), dict(F=0), dict(n=0), dict(n=-1), dict(n_slots=0), dict(n_slots=-3), dict(h=0), dict(w=0),
               dict(xd3_hi=None), dict(xd3_lo=None)):
        assert f(ctypes.byref(_args(**kw)), None) == lib.E_DIM, kw
    assert f(ctypes.byref(_args(feat_dtype=7)), None) == lib.E_DTYPE
    for kw in (dict(feat=40), dict(pool_feat=100), dict(xd3_hi=72), dict(pool_xd3_lo=152), dict(gmm=50), dict(pool_gmm=114), dict(slots=18)):
        assert f(ctypes.byref(_args(**kw)), None) == lib.E_ALIGN, kw
    # (mu, sigma) frames and the table are only 4-byte aligned: these pass the checks of the cases above (nothing is launched here:
    # a pool left out with its source is simply skipped, and a call without any source launches nothing)
    none = _args(feat=None, gmm=None, xd3_hi=None, xd3_lo=None, pool_gmm=116, slots=20)
    assert f(ctypes.byref(none), None) == 0


def test_scatter_frames_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    n, n_slots, h, w, F = 2, 4, 5, 7, 16
    R = (h + 2) * (w + 2)
    slots = torch.zeros(n, dtype=torch.int32)
    pool_feat, feat = torch.zeros(n_slots, h + 2, w + 2, F), torch.zeros(n, h + 2, w + 2, F)
    with pytest.raises(lib.MagnetError, match="GPU only"):                          # no CPU fallback
        lib.scatter_frames(slots, pool_feat=pool_feat, feat=feat)
    with pytest.raises(lib.MagnetError, match="expected a torch.Tensor"):
        lib.scatter_frames([0, 1], pool_feat=pool_feat, feat=feat)
    if not torch.cuda.is_available():
        return                                                                         # the shape checks need tensors that pass the device check
    dev = torch.device("cuda:0")
    slots, pool_feat, feat = slots.to(dev), pool_feat.to(dev), feat.to(dev)
    pool_gmm, gmm = torch.zeros(n_slots, 2, h, w, device=dev), torch.zeros(n, 2, h, w, device=dev)
    planes = lambda k: tuple(torch.zeros(k, R, 256, dtype=torch.bfloat16, device=dev) for _ in range(2))
    bad = [
        (dict(slots=slots.long()), "dtype"), (dict(slots=slots.view(1, n)), "slots has shape"),
        (dict(feat=feat[:1]), "feat has shape"), (dict(feat=feat.bfloat16()), "dtype"), (dict(pool_feat=None), "feat needs pool_feat"),
        (dict(gmm=gmm[:1]), "gmm has shape"), (dict(gmm=gmm.double()), "dtype"), (dict(pool_gmm=None), "gmm needs pool_gmm"),
        (dict(pool_gmm=torch.zeros(n_slots + 1, 2, h, w, device=dev)), "slots of"),
        (dict(xd3=planes(n + 1)), "xd3 hi plane has shape"), (dict(pool_xd3=planes(n_slots + 1)), "pool_xd3 hi plane has shape"),
        (dict(xd3=tuple(p.float() for p in planes(n))), "dtype"), (dict(pool_xd3=None), "xd3 needs pool_xd3"),
        (dict(feat=None, gmm=None), "do not carry h and w"), (dict(feat=None, gmm=None, xd3=None), "no source given"),
    ]
    for kw, msg in bad:
        a = dict(slots=slots, pool_feat=pool_feat, pool_gmm=pool_gmm, pool_xd3=planes(n_slots), feat=feat, gmm=gmm, xd3=planes(n))
        a.update(kw)
        with pytest.raises(lib.MagnetError, match=msg):
            lib.scatter_frames(a.pop("slots"), **a)


def test_sequence_runner_takes_graph_as_a_bool_only():
    args = make_args(D=5, iters=1, dpv_h=8, dpv_w=8, fdim=16, V=2)
    model = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=16)).eval()
    for bad in (1, 0, "yes", None):
        with pytest.raises(lib.MagnetError, match="graph"):
            SequenceRunner(model, 4, graph=bad)
    assert SequenceRunner(model, 4).graph_stats is None and SequenceRunner(model, 4, graph=False).graph_stats is None
    stats = SequenceRunner(model, 4, graph=True).graph_stats
    assert stats == {"captures": {}, "replays": {}}
