"""CPU: synchronised BatchNorm for the F-Net's HIP training path (magnet_amd/train_fnet.py, magnet_bn_sync_* of the C ABI): the new
exports and their prototypes, the argument-error codes of each entry point, the rank-order merge of (n, mean, M2) records in fp64
against numpy over the concatenated data, and the runner's decision table (when a BatchNorm slot synchronises)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from magnet_amd import fnet, lib, train_fnet

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("magnet_bn_sync_moments", "magnet_bn_sync_merge", "magnet_bn_sync_backward_sums", "magnet_bn_sync_backward_apply")


def test_exports_are_declared_and_bound(hip_lib):
    hdr = open(os.path.join(REPO, "include", "magnet_hip.h")).read()
    for name in NEW:
        assert name in lib._PROTOS and name in lib.API_SYMBOLS, name
        assert re.search(r"^MAGNET_API int %s\(" % name, hdr, flags=re.M), name
        assert hasattr(hip_lib, name), name
    syms = list(lib.API_SYMBOLS)
    assert syms.index(NEW[-1]) + 1 == syms.index("magnet_dnet_loss_workspace")            # in front of the D-Net loss entries
    assert int(re.search(r"#define\s+MAGNET_HIP_VERSION\s+(\d+)", hdr).group(1)) == 500 == hip_lib.magnet_version()


def _fwd_args():
    a = lib.MagnetBnTrainArgs()
    a.x, a.work, a.mean, a.invstd = 16, 16, 16, 16
    a.N, a.hp, a.wp, a.pad, a.C, a.x_ld = 1, 1, 1, 0, 16, 16                             # ONE position: valid under sync
    a.eps, a.momentum = 1e-5, 0.1
    return a


def _bwd_args():
    b = lib.MagnetBnBwdArgs()
    b.x = b.mean = b.invstd = b.gamma = b.beta = b.g = b.work = b.dgamma = b.dbeta = b.dx_hi = b.dx_lo = 16
    b.N, b.hp, b.wp, b.pad, b.C, b.x_ld, b.g_ld, b.dx_ld = 1, 1, 1, 0, 16, 16, 16, 16
    return b


def test_argument_errors_are_codes(hip_lib):
    """NULL buffers -> MAGNET_E_NULL, world = 0 and C = 12 -> MAGNET_E_DIM, each before any HIP call (the pointers are not memory)."""
    E_NULL, E_DIM = lib.E_NULL, lib.E_DIM
    mom, mrg, bsum, bapp = (getattr(hip_lib, n) for n in NEW)
    a, b = _fwd_args(), _bwd_args()
    # NULL buffers
    assert mom(None, 16, None) == E_NULL and mom(ctypes.byref(a), None, None) == E_NULL
    assert mrg(None, 16, 2, 16, None) == E_NULL and mrg(ctypes.byref(a), None, 2, 16, None) == E_NULL
    assert mrg(ctypes.byref(a), 16, 2, None, None) == E_NULL
    assert bsum(None, 16, None) == E_NULL and bsum(ctypes.byref(b), None, None) == E_NULL
    assert bapp(None, 16, 2, 16, None) == E_NULL and bapp(ctypes.byref(b), None, 2, 16, None) == E_NULL
    assert bapp(ctypes.byref(b), 16, 2, None, None) == E_NULL
    a.work = None
    assert mom(ctypes.byref(a), 16, None) == E_NULL
    a = _fwd_args(); a.mean = None
    assert mrg(ctypes.byref(a), 16, 2, 16, None) == E_NULL
    b.dgamma = None
    assert bsum(ctypes.byref(b), 16, None) == E_NULL
    b = _bwd_args(); b.dx_lo = None
    assert bapp(ctypes.byref(b), 16, 2, 16, None) == E_NULL
    # world = 0
    a, b = _fwd_args(), _bwd_args()
    assert mrg(ctypes.byref(a), 16, 0, 16, None) == E_DIM and b"world" in hip_lib.magnet_last_error()
    assert bapp(ctypes.byref(b), 16, 0, 16, None) == E_DIM and b"world" in hip_lib.magnet_last_error()
    # C = 12 (not a multiple of 8) and C above 2048
    for C in (12, 2056):
        a, b = _fwd_args(), _bwd_args()
        a.C = a.x_ld = C
        b.C = b.x_ld = b.g_ld = b.dx_ld = C
        assert mom(ctypes.byref(a), 16, None) == E_DIM, C
        assert mrg(ctypes.byref(a), 16, 2, 16, None) == E_DIM, C
        assert bsum(ctypes.byref(b), 16, None) == E_DIM, C
        assert bapp(ctypes.byref(b), 16, 2, 16, None) == E_DIM, C
    # the single-process statistics still need two positions; the apply, which takes its statistics as given, needs one
    a = _fwd_args()
    assert hip_lib.magnet_bn_train_stats(ctypes.byref(a), None) == E_DIM


# ---- the merge --------------------------------------------------------------------------------------------------------------------
def _records(shards):
    """[(n, mean, M2)] of one channel's shards, each computed on the shard alone (numpy fp64, two-pass)."""
    return [(float(len(s)), float(np.mean(s)), float(np.sum((s - np.mean(s)) ** 2))) for s in shards]


def _check_merge(shards):
    """Bound: the records carry the two-pass rounding of their shard (a few n eps relative to M2_r, eps |mean_r|); the merge adds
    world terms; (mean_r - mean)^2 carries 2 eps |mean| |mean_r - mean|.  With n <= 300, |mean| <= 1.1e3 and M2 / n >= 1 here,
    1e-11 relative on M2 and 1e-13 on the mean leave two orders of margin and sit eleven orders below the fp32 statistics."""
    n_tot, mean, M2 = train_fnet.bn_merge_records(_records(shards))
    allx = np.concatenate(shards)
    assert n_tot == len(allx)
    assert abs(mean - np.mean(allx)) <= 1e-13 * max(abs(np.mean(allx)), 1.0)
    exp = float(np.sum((allx - np.mean(allx)) ** 2))
    assert abs(M2 - exp) <= 1e-11 * exp
    return n_tot, mean, M2


def test_merge_matches_numpy_over_the_concatenated_data():
    rng = np.random.default_rng(0)
    _check_merge([rng.standard_normal(200) * 3 + 5, rng.standard_normal(37) * 3 + 5, rng.standard_normal(1) * 3 + 5])   # unequal
    # one value per channel on a shard: M2_r = 0, the variance comes from the means alone
    one = [np.array([4.25]), np.array([-1.5])]
    assert _records(one)[0][2] == 0.0 and _records(one)[1][2] == 0.0
    n, mean, M2 = _check_merge(one)
    assert (n, mean) == (2.0, 1.375) and M2 == 2 * 2.875 ** 2
    # |mean| >> std, one shard offset by +100
    _check_merge([rng.standard_normal(150) * 1e-2 + 1000.0, rng.standard_normal(90) * 1e-2 + 1100.0])
    _check_merge([rng.standard_normal(64) * 3 + 5, rng.standard_normal(64) * 3 + 105, rng.standard_normal(3) * 3 + 5])


def test_merge_then_running_update_is_batchnorm_over_the_whole_batch():
    """merge + bn_running_update on two shards = nn.BatchNorm2d (fp64) on the concatenated batch, momentum 0.1 and None."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 8, 5, 7, dtype=torch.float64, generator=g) * 2 + 1
    x[2] += 100
    for momentum in (0.1, None):
        bn = nn.BatchNorm2d(8, momentum=momentum).double().train()
        bn.running_mean.normal_(generator=g); bn.running_var.uniform_(0.5, 2.0, generator=g); bn.num_batches_tracked.fill_(3)
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        bn(x)
        for c in range(8):
            shards = [x[:2, c].reshape(-1).numpy(), x[2:, c].reshape(-1).numpy()]
            n, mean, M2 = train_fnet.bn_merge_records(_records(shards))
            erm, erv, nbt = train_fnet.bn_running_update(float(rm[c]), float(rv[c]), mean, M2 / n, n, momentum, 3)
            assert math.isclose(erm, float(bn.running_mean[c]), rel_tol=1e-12, abs_tol=1e-12)
            assert math.isclose(erv, float(bn.running_var[c]), rel_tol=1e-12)
            assert nbt == int(bn.num_batches_tracked) == 4


# ---- the decision table -----------------------------------------------------------------------------------------------------------
class _FakeDist:
    """torch.distributed as sync_group sees it: initialised or not, and a world size per group."""

    class group:
        WORLD = "world"

    def __init__(self, initialised, sizes):
        self.initialised, self.sizes = initialised, sizes

    def is_available(self):
        return True

    def is_initialized(self):
        return self.initialised

    def get_world_size(self, group=None):
        return self.sizes[group]


def test_sync_group_decision_table(monkeypatch):
    sbn, bn = nn.SyncBatchNorm(8), nn.BatchNorm2d(8)
    sub = nn.SyncBatchNorm(8, process_group="pair")
    solo = nn.SyncBatchNorm(8, process_group="solo")
    # no process group initialised: today's path for every module (the real torch.distributed of this process)
    assert not torch.distributed.is_initialized()
    for m in (sbn, bn, sub):
        assert train_fnet.sync_group(m) is None
    monkeypatch.setattr(train_fnet, "dist", _FakeDist(True, {"world": 2, "pair": 2, "solo": 1}))
    assert train_fnet.sync_group(sbn) == "world"                      # process_group None: the default group
    assert train_fnet.sync_group(sub) == "pair"
    assert train_fnet.sync_group(solo) is None                        # a one-rank group
    assert train_fnet.sync_group(bn) is None                          # plain BatchNorm2d never synchronises
    assert train_fnet.sync_group(sbn.eval()) is None                  # .eval()
    assert train_fnet.sync_group(sbn.train()) == "world"
    monkeypatch.setattr(train_fnet, "dist", _FakeDist(True, {"world": 1}))
    assert train_fnet.sync_group(sbn) is None                         # a one-rank default group
    monkeypatch.setattr(train_fnet, "dist", _FakeDist(False, {}))
    assert train_fnet.sync_group(sbn) is None


def test_check_input_under_sync(monkeypatch):
    """One 256 x 256 image pools to one branch1 cell: refused alone, accepted when the statistics come from several ranks; the
    affine check sees SyncBatchNorm modules (not a subclass of BatchNorm2d)."""
    psm = nn.SyncBatchNorm.convert_sync_batchnorm(fnet.PSMNet(feature_dim=32))
    assert isinstance(psm.branch1[1][1], nn.SyncBatchNorm) and not isinstance(psm.branch1[1][1], nn.BatchNorm2d)
    img = torch.zeros(1, 3, 256, 256)
    with pytest.raises(lib.MagnetError, match="at least 2 values"):
        train_fnet.check_input(img, psm)
    with pytest.raises(lib.MagnetError, match="must be on the GPU"):  # the last check: every shape check passed
        train_fnet.check_input(img, psm, sync=True)
    with pytest.raises(lib.MagnetError, match="at least 2 values"):   # no process group: a SyncBatchNorm F-Net takes today's path
        train_fnet.FNetTrainHIP(psm).run(img)
    monkeypatch.setattr(train_fnet, "dist", _FakeDist(True, {"world": 2}))
    with pytest.raises(lib.MagnetError, match="must be on the GPU"):
        train_fnet.FNetTrainHIP(psm).run(img)
    psm.layer1[0].conv2[1] = nn.SyncBatchNorm(32, affine=False)
    with pytest.raises(lib.MagnetError, match="without affine"):
        train_fnet.check_input(torch.zeros(2, 3, 256, 256), psm)
