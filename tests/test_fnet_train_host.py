"""CPU: MAGNET_F's constructor (f_net=None builds the state_dict-compatible FNET, train_backend validation), the checks the HIP
F-Net training path makes before any launch, the running-statistics update it implements, the input-gradient weight packs and the
space-to-depth weight-gradient mapping in fp64, and the C layout of the new argument structs."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from magnet_amd import fnet, lib, train_fnet
from magnet_amd.magnet import MAGNET_F

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class _Args:
    FNET_architecture = "PSM-Net"
    FNET_feature_dim = 64


def test_magnet_f_builds_fnet_with_reference_keys():
    m = MAGNET_F(_Args())
    assert isinstance(m.f_net, fnet.FNET) and m.train_backend == "torch"
    sd = m.state_dict()
    psm_keys = set(fnet.PSMNet(feature_dim=64).state_dict())
    assert len(sd) == 361 and {k[len("f_net.f_net."):] for k in sd} == psm_keys      # reference: MAGNET_F.f_net = FNET(args)
    for k in ("f_net.f_net.firstconv.0.0.weight", "f_net.f_net.layer2.0.downsample.1.bias", "f_net.f_net.branch3.1.0.weight",
              "f_net.f_net.lastconv.2.weight"):
        assert k in sd, k
    assert sd["f_net.f_net.lastconv.2.weight"].shape == (64, 128, 1, 1)


def test_magnet_f_keeps_a_given_module_and_checks_backend():
    given = fnet.FNET(_Args())
    assert MAGNET_F(_Args(), given).f_net is given
    assert MAGNET_F(_Args(), f_net=given, train_backend="hip").train_backend == "hip"
    with pytest.raises(lib.MagnetError, match="train_backend"):
        MAGNET_F(_Args(), train_backend="bogus")
    with pytest.raises(lib.MagnetError, match="train_backend"):
        MAGNET_F(_Args(), given, train_backend="cuda")


def test_hip_backend_trains_on_the_gpu_only():
    """Grad enabled, trainable F-Net, .train(): the HIP autograd path runs its checks (no quiet fall-back to torch on the CPU)."""
    m = MAGNET_F(_Args(), train_backend="hip").train()
    img = torch.zeros(1, 3, 256, 256)
    with pytest.raises(lib.MagnetError, match="GPU"):
        m._features_hip(torch.cat([img, img]))
    with pytest.raises(lib.MagnetError, match="input images"):
        m._features_hip(torch.cat([img, img]).requires_grad_())


def _bf16_exact(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).double()


@pytest.mark.parametrize("dil", [1, 2])
def test_flipped_dgrad_pack_fp64(dil):
    """conv(dz, flipped transposed 3x3 pack, same dilation and padding) == conv2d_input, in fp64 (bf16-exact weights: lo = 0)."""
    w = _bf16_exact(16, 8, 3, 3, seed=dil)
    dz = torch.randn(2, 16, 9, 11, dtype=torch.float64)
    hi, lo = train_fnet.dgrad_pack(w.float())
    assert not lo.float().any()
    wt = hi.double().reshape(3, 3, 8, 16).permute(2, 3, 0, 1)                     # (cin, cout, ky, kx)
    got = torch.nn.functional.conv2d(dz, wt, padding=dil, dilation=dil)
    exp = torch.nn.grad.conv2d_input((2, 8, 9, 11), w, dz, padding=dil, dilation=dil)
    torch.testing.assert_close(got, exp, rtol=1e-12, atol=1e-12)


def _s2d(x):
    return torch.cat([x[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=1)


def test_s2d_mirrored_window_and_downsample_fp64():
    """The stride-2 layers' input gradient: the mirrored 2x2 window over the space-to-depth grid (the window read one row and one
    column further), plus the phase-0 1x1 downsample, then depth-to-space == conv2d_input of the stride-2 3x3 and 1x1, in fp64."""
    C, cout, H, W = 8, 16, 10, 14
    w = _bf16_exact(cout, C, 3, 3, seed=3)
    wd = _bf16_exact(cout, C, 1, 1, seed=4)
    gz = torch.randn(2, cout, H // 2, W // 2, dtype=torch.float64)
    gzd = torch.randn(2, cout, H // 2, W // 2, dtype=torch.float64)
    hi, lo = train_fnet.dgrad_pack_s2d(w.float())                                  # (4, 4C, cout)
    assert not lo.float().any()
    k = hi.double().reshape(2, 2, 4 * C, cout).permute(2, 3, 0, 1)                 # tap t = a*2+b reads dz[y + a, x + b]
    dS = torch.nn.functional.conv2d(torch.nn.functional.pad(gz, (0, 1, 0, 1)), k)
    hd, _ = train_fnet.dgrad_pack(wd.float())
    dS[:, :C] += torch.einsum("co,nohw->nchw", hd.double()[0], gzd)                 # phase-0 channels only
    got = torch.empty(2, C, H, W, dtype=torch.float64)
    for ph, (py, px) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        got[:, :, py::2, px::2] = dS[:, ph * C:(ph + 1) * C]
    exp = torch.nn.grad.conv2d_input((2, C, H, W), w, gz, stride=2, padding=1) + \
        torch.nn.grad.conv2d_input((2, C, H, W), wd, gzd, stride=2)
    torch.testing.assert_close(got, exp, rtol=1e-12, atol=1e-12)


def test_s2d_weight_gradient_mapping_fp64():
    """The 2x2-window weight gradient over the space-to-depth input, mapped back, == conv2d_weight of the stride-2 3x3."""
    C, cout, H, W = 8, 16, 10, 14
    x = torch.randn(2, C, H, W, dtype=torch.float64)
    gz = torch.randn(2, cout, H // 2, W // 2, dtype=torch.float64)
    s = torch.nn.functional.pad(_s2d(x), (1, 0, 1, 0))                             # the window reaches (-1, -1)
    g4 = torch.nn.grad.conv2d_weight(s, (cout, 4 * C, 2, 2), gz)
    got = train_fnet.s2d_grad_to_3x3(g4, C)
    exp = torch.nn.grad.conv2d_weight(x, (cout, C, 3, 3), gz, stride=2, padding=1)
    torch.testing.assert_close(got, exp, rtol=1e-12, atol=1e-12)


def test_training_forward_input_checks():
    psm = fnet.PSMNet(feature_dim=64)
    ok = torch.zeros(2, 3, 256, 256)
    with pytest.raises(lib.MagnetError, match="GPU"):
        train_fnet.check_input(ok, psm)                         # the shapes are fine: only the device is wrong
    with pytest.raises(lib.MagnetError, match="too small"):
        train_fnet.check_input(torch.zeros(2, 3, 252, 256), psm)                     # H/4 = 63
    with pytest.raises(lib.MagnetError, match="2 values per channel"):
        train_fnet.check_input(torch.zeros(1, 3, 256, 320), psm)                     # branch1: one cell
    with pytest.raises(lib.MagnetError, match=r"\(N, 3, H, W\)"):
        train_fnet.check_input(torch.zeros(2, 1, 256, 256), psm)
    with pytest.raises(lib.MagnetError, match="feature_dim"):
        train_fnet.check_input(ok, fnet.PSMNet(feature_dim=48))
    with pytest.raises(lib.MagnetError, match="GPU"):
        with torch.no_grad():                                   # .train() under no_grad reaches the checks, then refuses the CPU
            MAGNET_F(_Args(), train_backend="hip").train()._features_hip(ok)


@pytest.mark.parametrize("struct", ["MagnetWgradExArgs", "MagnetBnBwdArgs", "MagnetSppBwdArgs"])
def test_backward_structs_layout_matches_c(struct):
    A = getattr(lib, struct)
    fields = [f[0] for f in A._fields_]
    header = os.path.join(REPO, "include", "magnet_hip.h")
    prog = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(%s));' % (header, struct)
    for f in fields:
        prog += 'printf(" %%zu", offsetof(%s, %s));' % (struct, f)
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert vals[0] == ctypes.sizeof(A)
    assert vals[1:] == [getattr(A, f).offset for f in fields]


@pytest.mark.parametrize("momentum", [0.1, 0.3, None])
def test_running_update_matches_torch(momentum):
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm2d(8, momentum=momentum).double().train()
    bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0); bn.num_batches_tracked.fill_(3)
    x = torch.randn(3, 8, 5, 7, dtype=torch.float64) * 2 + 1
    rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)
    bn(x)
    n = x.numel() // 8
    mean = x.mean(dim=(0, 2, 3))
    var = x.var(dim=(0, 2, 3), unbiased=False)
    erm, erv, enbt = train_fnet.bn_running_update(rm, rv, mean, var, n, momentum, nbt)
    torch.testing.assert_close(erm, bn.running_mean, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(erv, bn.running_var, rtol=1e-13, atol=1e-13)
    assert enbt == int(bn.num_batches_tracked) == 4


def test_bn_train_args_layout_matches_c():
    A = lib.MagnetBnTrainArgs
    fields = [f[0] for f in A._fields_]
    header = os.path.join(REPO, "include", "magnet_hip.h")
    prog = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(MagnetBnTrainArgs));' % header
    for f in fields:
        prog += 'printf(" %%zu", offsetof(MagnetBnTrainArgs, %s));' % f
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert vals[0] == ctypes.sizeof(A)
    assert vals[1:] == [getattr(A, f).offset for f in fields]


def test_bn_train_argument_errors_are_codes(hip_lib):
    assert hip_lib.magnet_bn_train_stats(None, None) == 1                        # MAGNET_E_NULL
    a = lib.MagnetBnTrainArgs()
    assert hip_lib.magnet_bn_train_apply(ctypes.byref(a), None) == 1
    a.x, a.mean, a.invstd, a.work = 16, 16, 16, 16
    a.N, a.hp, a.wp, a.pad, a.C, a.x_ld = 1, 4, 4, 1, 12, 12                     # C % 8 != 0
    assert hip_lib.magnet_bn_train_stats(ctypes.byref(a), None) == 2             # MAGNET_E_DIM
    a.C, a.x_ld, a.hp, a.wp = 16, 16, 3, 3                                       # one interior position
    assert hip_lib.magnet_bn_train_stats(ctypes.byref(a), None) == 2
    assert hip_lib.magnet_fnet_stem_raw(None, None, None, 1, 8, 8, None) == 1
