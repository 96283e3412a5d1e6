"""Host-side checks of the HIP training path (no GPU needed): MagnetLoss's interface, MAGNET(train_backend=...), and the new
C entry points (declared, exported, NULL arguments come back as MAGNET_E_NULL)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from magnet_amd import lib
from magnet_amd.standin import StubDNet, StubFNet, make_args

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("magnet_nll_loss_forward", "magnet_nll_loss_backward", "magnet_upsample_depth_backward", "magnet_head_dgrad",
       "magnet_wgrad_workspace", "magnet_wgrad")


def test_magnet_loss_reads_args_and_rejects_other_loss_fns():
    from magnet_amd.losses import MagnetLoss
    m = MagnetLoss(SimpleNamespace(loss_fn="gaussian", loss_gamma=0.7))
    assert m.loss_type == "gaussian" and m.gamma == 0.7
    bad = MagnetLoss(SimpleNamespace(loss_fn="l1", loss_gamma=0.8))
    with pytest.raises(lib.MagnetError):
        bad([torch.zeros(1, 2, 4, 4)], torch.zeros(1, 1, 4, 4), torch.ones(1, 1, 4, 4, dtype=torch.bool))


def test_magnet_loss_has_no_cpu_fallback():
    from magnet_amd.losses import MagnetLoss
    m = MagnetLoss(SimpleNamespace(loss_fn="gaussian", loss_gamma=0.8))
    with pytest.raises(lib.MagnetError, match="CPU fallback"):
        m([torch.rand(1, 2, 4, 4)], torch.rand(1, 1, 4, 4), torch.ones(1, 1, 4, 4, dtype=torch.bool))


def test_train_backend_argument():
    from magnet_amd.magnet import MAGNET
    args = make_args(D=5, iters=2, dpv_h=12, dpv_w=16)
    m = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8), train_backend="hip")
    assert m.train_backend == "hip"
    assert MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8)).train_backend == "torch"
    with pytest.raises(lib.MagnetError, match="train_backend"):
        MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8), train_backend="triton")


def test_new_entry_points_declared_and_exported(hip_lib):
    src = open(os.path.join(REPO, "include", "magnet_hip.h")).read()
    declared = set(re.findall(r"MAGNET_API\s+[\w\s\*]+?\b(magnet_\w+)\s*\(", src))
    for s in NEW:
        assert s in declared and s in lib.API_SYMBOLS and hasattr(hip_lib, s), s
    assert hip_lib.magnet_version() == 500


def test_new_entry_points_return_null_codes(hip_lib):
    for name, st in (("magnet_nll_loss_forward", lib.MagnetNllArgs), ("magnet_nll_loss_backward", lib.MagnetNllArgs),
                     ("magnet_upsample_depth_backward", lib.MagnetUpsampleBwdArgs), ("magnet_head_dgrad", lib.MagnetHeadDgradArgs),
                     ("magnet_wgrad", lib.MagnetWgradArgs)):
        f = getattr(hip_lib, name)
        assert f(None, None) == lib.E_NULL, name
        a = st()                                    # all zero: every pointer NULL
        assert f(ctypes.byref(a), None) == lib.E_NULL, name
        assert b"NULL" in hip_lib.magnet_last_error()
    assert hip_lib.magnet_wgrad_workspace(None) == -lib.E_NULL
    assert hip_lib.magnet_wgrad_workspace(ctypes.byref(lib.MagnetWgradArgs())) == -lib.E_NULL


def test_new_entry_points_return_dim_codes(hip_lib):
    a = lib.MagnetWgradArgs(dy_hi=16, dy_lo=16, x_hi=16, x_lo=16, grad_w=16, work=16, dy_ld=8, x_ld=8, rows=100, cout=7, cin=8,
                            taps=1, wp=6, cout_valid=7, cin_valid=8, cin_total=8)
    assert hip_lib.magnet_wgrad(ctypes.byref(a), None) == lib.E_DIM          # cout % 8
    n = lib.MagnetNllArgs(preds=16, gt=16, mask=16, sums=16, loss=16, work=16, n_iter=17, B=1, H=1, W=1)
    assert hip_lib.magnet_nll_loss_forward(ctypes.byref(n), None) == lib.E_DIM


@pytest.mark.parametrize("struct", ["MagnetNllArgs", "MagnetUpsampleBwdArgs", "MagnetHeadDgradArgs", "MagnetWgradArgs"])
def test_new_struct_layouts_match_c(struct, tmp_path):
    import subprocess
    A = getattr(lib, struct)
    fields = [f[0] for f in A._fields_]
    prog = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(%s));' % (
        os.path.join(REPO, "include", "magnet_hip.h"), struct)
    for f in fields:
        prog += 'printf(" %%zu", offsetof(%s, %s));' % (struct, f)
    prog += "return 0;}\n"
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(prog)
    subprocess.check_call(["gcc", str(c), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == ctypes.sizeof(A)
    assert vals[1:] == [getattr(A, f).offset for f in fields]
