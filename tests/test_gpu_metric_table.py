"""magnet_depth_metrics_ex, MetricTable and the sharded evaluation drivers on the GPU.

SIGMA sums are compared with magnet_depth_metrics[_crop] to the bit; VARIANCE and NONE with the float64 restatement of
tests/metrics_ref.py inside its derived bounds; the per-frame rows with metrics.metrics_from_sums of the device sums as float.hex()
strings; the drivers' validate_sharded with their validate()."""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DMIN, DMAX = 1e-3, 10.0
# (1, 129, 128): 16 512 pixels, one more grid-stride pass for the first 128 threads of stage 1 (64 workgroups x 256 threads)
SHAPES = [(1, 1, 1), (1, 1, 5), (3, 7, 13), (2, 64, 96), (1, 129, 128)]
SENTINEL = -7.25


def _seed(shape, kind):
    return 1000 * kind + shape[1] * shape[2]                   # the seeds tests/test_metric_table_host.py checks the margins of


@lru_cache(maxsize=None)
def _case(shape, kind):
    """Seeded host inputs and their restated sums / bounds per frame (computed once, shared, never modified)."""
    mu, second, gt = R.make_case(*shape, kind, _seed(shape, kind))
    ref = [R.frame_sums(mu[b], None if second is None else second[b], gt[b], kind, DMIN, DMAX) for b in range(shape[0])]
    for a in (mu, second, gt):
        if a is not None:
            a.setflags(write=False)
    return mu, second, gt, ref


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def _ex(mu, second, gt, kind, window=None, want_sums=True, rows=None, row0=0):
    """One magnet_depth_metrics_ex call on device tensors mu / second (B,H,W views with contiguous planes) and gt (B,H,W) contiguous.
    rows: a (n,12) float64 device tensor, written from row `row0`.  Returns the (B,16) sums (or None)."""
    from magnet_amd import lib as L
    B, H, W = mu.shape
    a = L.MagnetDepthMetricsArgs()
    a.mu, a.mu_stride, a.gt = mu.data_ptr(), (mu.stride(0) if B > 1 else H * W), gt.data_ptr()
    if second is not None:
        a.second, a.second_stride = second.data_ptr(), (second.stride(0) if B > 1 else H * W)
    a.B, a.H, a.W, a.kind = B, H, W, kind
    a.min_depth, a.max_depth = DMIN, DMAX
    if window is not None:
        a.crop, (a.y0, a.y1, a.x0, a.x1) = 1, window
    sums = torch.full((B, 16), SENTINEL, dtype=torch.float64, device=mu.device) if want_sums else None
    if sums is not None:
        a.sums = sums.data_ptr()
    if rows is not None:
        assert row0 + B <= rows.shape[0]
        a.rows = rows.data_ptr() + row0 * 12 * 8
    work = torch.empty(int(L.load().magnet_depth_metrics_workspace(B)) // 8, dtype=torch.float64, device=mu.device)
    a.work = work.data_ptr()
    L._launch("magnet_depth_metrics_ex", mu, ctypes.byref(a))
    return sums


def _hex(t):
    return [[float(v).hex() for v in row] for row in t.cpu().tolist()]


@pytest.mark.parametrize("shape", SHAPES)
def test_sigma_sums_equal_depth_metric_sums_to_the_bit(hip_lib, gpu, shape):
    """As the two channels of one (B,2,H,W) tensor and as separately allocated planes."""
    from magnet_amd import metrics as M
    mu, sg, gt, _ = _case(shape, R.SIGMA)
    pred = torch.stack([_dev(mu, gpu), _dev(sg, gpu)], dim=1)
    g = _dev(gt, gpu)
    want = M.depth_metric_sums(pred, g, DMIN, DMAX)
    got = _ex(pred[:, 0], pred[:, 1], g, R.SIGMA)
    assert _hex(got) == _hex(want)
    apart = _ex(pred[:, 0].contiguous(), pred[:, 1].clone().contiguous(), g, R.SIGMA)
    assert _hex(apart) == _hex(want)
    assert float(want[:, 0].min()) >= 1


@pytest.mark.parametrize("crop", ["garg", "eigen"])
def test_sigma_sums_with_the_kitti_crops(hip_lib, gpu, crop):
    from magnet_amd import metrics as M
    shape = (1, 40, 120)
    mu, sg, gt = R.make_case(*shape, R.SIGMA, 77)
    pred = torch.stack([_dev(mu, gpu), _dev(sg, gpu)], dim=1)
    g = _dev(gt, gpu)
    win = M.crop_window(crop, 40, 120)
    want = M.depth_metric_sums(pred, g, DMIN, DMAX, crop=crop)
    assert _hex(_ex(pred[:, 0], pred[:, 1], g, R.SIGMA, window=win)) == _hex(want)
    assert _hex(_ex(pred[:, 0].contiguous(), pred[:, 1].contiguous(), g, R.SIGMA, window=win)) == _hex(want)
    whole = M.depth_metric_sums(pred, g, DMIN, DMAX)
    assert 0 < float(want[0, 0]) < float(whole[0, 0])
    ref, bound = R.frame_sums(mu[0], sg[0], gt[0], R.SIGMA, DMIN, DMAX, window=win)
    assert np.all(np.abs(want[0, :13].cpu().numpy() - ref) <= bound)


def _within(got, ref, bound):
    d = np.abs(got - ref)
    for k in range(13):
        print(f"  sum {k:2d}: device {got[k]:.17g} restated {ref[k]:.17g} |diff| {d[k]:.3e} bound {bound[k]:.3e}")
    return bool(np.all(d <= bound))


@pytest.mark.parametrize("shape", SHAPES)
def test_variance_sums_within_the_bounds(hip_lib, gpu, shape):
    """The variance plane is clamped as it is.  The route the driver took before (sqrt in fp32, then SIGMA squares it again) misses
    the nll bound on the same inputs wherever there are enough pixels for fp32's rounding of the root not to vanish by chance."""
    mu, var, gt, ref = _case(shape, R.VARIANCE)
    m, v, g = _dev(mu, gpu), _dev(var, gpu), _dev(gt, gpu)
    got = _ex(m, v, g, R.VARIANCE).cpu().numpy()
    old = _ex(m, torch.sqrt(v), g, R.SIGMA).cpu().numpy()
    for b in range(shape[0]):
        s, bound = ref[b]
        assert _within(got[b, :13], s, bound), (shape, b)
        assert all(got[b, k] == s[k] for k in (0, 9, 10, 11)) and np.all(got[b, 13:] == 0.0)
        print(f"  sqrt route: nll sum off by {abs(old[b, 12] - s[12]):.3e}, bound {bound[12]:.3e}")
        assert np.all(np.abs(old[b, :12] - s[:12]) <= bound[:12])
        if s[0] >= 1000:
            assert abs(old[b, 12] - s[12]) > bound[12]


@pytest.mark.parametrize("shape", SHAPES)
def test_none_equals_sigma_without_the_nll(hip_lib, gpu, shape):
    mu, sg, gt, ref = _case(shape, R.SIGMA)
    m, s, g = _dev(mu, gpu), _dev(sg, gpu), _dev(gt, gpu)
    with_sigma = _ex(m, s, g, R.SIGMA)
    rows = torch.full((shape[0], 12), SENTINEL, dtype=torch.float64, device=gpu)
    none = _ex(m, None, g, R.NONE, rows=rows)
    assert _hex(none[:, :12]) == _hex(with_sigma[:, :12])
    assert np.all(none[:, 12:].cpu().numpy() == 0.0)
    assert all(v == "0x0.0p+0" for v in (r[11] for r in _hex(rows)))
    for b in range(shape[0]):
        assert _within(with_sigma[b, :13].cpu().numpy(), *ref[b]), (shape, b)


def _want_rows(sums, kind):
    from magnet_amd import metrics as M
    out = []
    for s in sums.cpu().tolist():
        m = M.metrics_from_sums(s)
        if kind == R.NONE:
            m["nll"] = 0.0
        out.append([float(m[k]).hex() for k in M.METRIC_ORDER])
    return out


@pytest.mark.parametrize("kind", [R.SIGMA, R.VARIANCE, R.NONE])
@pytest.mark.parametrize("shape", SHAPES)
def test_rows_equal_metrics_from_sums(hip_lib, gpu, shape, kind):
    """Every row is metrics_from_sums of that frame's device sums, string for string; the rows in front of and behind the B written
    ones keep their sentinel; rows alone (no sums) and a second run give the same rows."""
    mu, second, gt, _ = _case(shape, kind)
    m, g = _dev(mu, gpu), _dev(gt, gpu)
    s = None if second is None else _dev(second, gpu)
    B = shape[0]
    rows = torch.full((B + 3, 12), SENTINEL, dtype=torch.float64, device=gpu)
    sums = _ex(m, s, g, kind, rows=rows, row0=1)
    got = _hex(rows)
    assert got[1:B + 1] == _want_rows(sums, kind)
    assert got[1:B + 1] == [[float(v).hex() for v in R.row_from_sums(row, kind)] for row in sums.cpu().tolist()]
    assert all(v == float(SENTINEL).hex() for r in (got[0], got[B + 1], got[B + 2]) for v in r)
    again = torch.full((B + 3, 12), SENTINEL, dtype=torch.float64, device=gpu)
    assert _ex(m, s, g, kind, want_sums=False, rows=again, row0=1) is None
    assert _hex(again) == got


@pytest.mark.parametrize("kind", [R.SIGMA, R.VARIANCE, R.NONE])
def test_frame_without_a_valid_pixel(hip_lib, gpu, kind):
    """NaN in all 12 entries; under NONE NaN in 11 and 0.0 in nll.  The frames around it are not touched by it."""
    shape = (3, 7, 13)
    mu, second, gt, _ = _case(shape, kind)
    gt = np.array(gt); gt[1] = 0.0
    m, g = _dev(mu, gpu), _dev(gt, gpu)
    s = None if second is None else _dev(second, gpu)
    rows = torch.full((3, 12), SENTINEL, dtype=torch.float64, device=gpu)
    sums = _ex(m, s, g, kind, rows=rows)
    assert np.all(sums[1].cpu().numpy() == 0.0)
    r = rows.cpu().tolist()
    assert all(math.isnan(v) for v in r[1][:11])
    assert r[1][11] == 0.0 and math.copysign(1.0, r[1][11]) == 1.0 if kind == R.NONE else math.isnan(r[1][11])
    assert _hex(rows) == _want_rows(sums, kind)
    assert all(math.isfinite(v) for b in (0, 2) for v in r[b])


def test_metric_table_grows_and_keeps_the_order(hip_lib, gpu):
    """5 appends of B = 2 into capacity 4: all 10 rows, in order, equal to the rows of one call per batch."""
    from magnet_amd import metrics as M
    mu, sg, gt = R.make_case(10, 7, 13, R.SIGMA, 21)
    pred = torch.stack([_dev(mu, gpu), _dev(sg, gpu)], dim=1)
    g = _dev(gt, gpu).unsqueeze(1)
    want = torch.full((10, 12), SENTINEL, dtype=torch.float64, device=gpu)
    for i in range(0, 10, 2):
        _ex(pred[i:i + 2, 0], pred[i:i + 2, 1], g[i:i + 2, 0].contiguous(), R.SIGMA, want_sums=False, rows=want, row0=i)
    table = M.MetricTable(gpu, DMIN, DMAX, capacity=4)
    assert len(table) == 0 and tuple(table.rows().shape) == (0, 12)
    for i in range(0, 10, 2):
        if i % 4:
            table.append_pred(pred[i:i + 2], g[i:i + 2])
        else:
            table.append(pred[i:i + 2, 0], g[i:i + 2], pred[i:i + 2, 1:2])
        assert len(table) == i + 2
    rows = table.rows()
    assert rows.is_cuda and rows.dtype == torch.float64 and tuple(rows.shape) == (10, 12)
    assert _hex(rows) == _hex(want)
    with pytest.raises(Exception, match="second plane"):
        table.append(pred[:2, 0], g[:2])


def test_metric_table_kinds_and_crop(hip_lib, gpu):
    from magnet_amd import metrics as M
    mu, var, gt = R.make_case(1, 40, 120, R.VARIANCE, 33)
    m, v, g = _dev(mu, gpu), _dev(var, gpu), _dev(gt, gpu)
    for kind, code, second in (("variance", R.VARIANCE, v), (None, R.NONE, None), ("sigma", R.SIGMA, v)):
        for crop in (None, "garg", "eigen", (3, 30, 10, 100)):
            win = M.crop_window(crop, 40, 120) if isinstance(crop, (str, type(None))) else crop
            want = torch.empty((1, 12), dtype=torch.float64, device=gpu)
            _ex(m, second, g, code, window=win, want_sums=False, rows=want)
            table = M.MetricTable(gpu, DMIN, DMAX, crop=crop, kind=kind, capacity=1)
            table.append(m, g, second)
            assert _hex(table.rows()) == _hex(want), (kind, crop)


def test_append_does_not_synchronise(hip_lib, gpu):
    """append and append_pred, the doubling included, under torch's sync debug mode; a control .item() in the same block must raise."""
    from magnet_amd import metrics as M
    mu, sg, gt = R.make_case(2, 7, 13, R.SIGMA, 4)
    pred = torch.stack([_dev(mu, gpu), _dev(sg, gpu)], dim=1)
    g = _dev(gt, gpu).unsqueeze(1)
    table = M.MetricTable(gpu, DMIN, DMAX, capacity=2)
    table.append_pred(pred, g)                                  # first call: library load, the work buffer of B = 2
    torch.cuda.synchronize()
    control = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        table.append_pred(pred, g)                              # doubles 2 -> 4
        table.append(pred[:, 0], g, pred[:, 1])                 # doubles 4 -> 8
        table.append(pred[:1, 0], g[:1], pred[:1, 1])           # a new B: its work buffer
        try:
            table.rows()[0, 0].item()
        except RuntimeError:
            control = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not control:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build: the test shows nothing")
    assert len(table) == 7
    r = _hex(table.rows())
    assert r[0:2] == r[2:4] == r[4:6] and r[6] == r[0]


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
def _hexdict(m):
    from magnet_amd import metrics as M
    return {k: float(m[k]).hex() for k in M.METRIC_ORDER}


def test_eval_synthetic_sharded_equals_validate(hip_lib, gpu):
    """The smallest MAGNET the GPU tests run (test_gpu_conv.py::test_eval_driver_runs), one NaN pose per batch, garg crop off / on."""
    sys.path.insert(0, REPO)
    import eval_synthetic as E
    from magnet_amd.magnet import MAGNET
    from tests.stubs import StubDNet, StubFNet, make_args, seeded_magnet_weights
    args = make_args(D=5, iters=2, dpv_h=12, dpv_w=16, V=2)
    args.min_depth, args.max_depth = 1e-3, 10.0
    model = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8))
    seeded_magnet_weights(model, 3)
    model = model.to(gpu).eval()
    for crop in (False, True):
        args.garg_crop, args.eigen_crop = crop, False
        want = E.validate(model, args, E.SyntheticWindows(3, 2, 2, 48, 64, nan_every=1), gpu)
        got, n = E.validate_sharded(model, args, E.SyntheticWindows(3, 2, 2, 48, 64, nan_every=1), gpu, with_count=True)
        assert n == 6 and _hexdict(got) == _hexdict(want)
        assert all(math.isfinite(v) for v in got.values())


def test_eval_fnet_sharded_equals_validate(hip_lib, gpu):
    """MAGNET_F at 480 x 640 (the only size the GPU tests run it at), V = 2, two windows: all 12 values, the nll 0.0 among them."""
    sys.path.insert(0, REPO)
    import eval_fnet as E
    from eval_synthetic import SyntheticWindows
    from magnet_amd.magnet import MAGNET_F
    args = argparse.Namespace(min_depth=1e-3, max_depth=10.0, garg_crop=False, eigen_crop=False, FNET_architecture="PSM-Net",
                              FNET_feature_dim=64)
    torch.manual_seed(0)
    model = MAGNET_F(args, train_backend="hip").to(gpu).eval()
    d_center = E.sid_centres(16, 1e-3, 10.0).to(gpu)
    want = E.validate(model, args, SyntheticWindows(2, 1, 2, 480, 640, seed=2), gpu, d_center)
    got = E.validate_sharded(model, args, SyntheticWindows(2, 1, 2, 480, 640, seed=2), gpu, d_center)
    assert _hexdict(got) == _hexdict(want) and got["nll"] == 0.0
    assert all(math.isfinite(v) for v in got.values())


def test_eval_dnet_sharded_against_validate_and_the_host_restatement(hip_lib, gpu):
    """11 values are validate()'s to the bit.  The nll comes from the variance itself: it lies within the bound of the float64
    restatement (tests/dnet_standalone_ref.py) and closer to it than validate()'s, which goes through an fp32 square root.
    The bound: per frame the kernel's nll sum is within metrics_ref's bound of the exact sum; the restatement's own np.mean carries a
    summation error of at most the same n 2^-53 sum|t|, which that bound contains - so twice the per-frame bound over n, averaged
    over the frames like the values themselves."""
    sys.path.insert(0, REPO)
    import eval_dnet as E
    from magnet_amd.standin import make_dnet
    from tests.dnet_standalone_ref import validate_host
    model = make_dnet(dnet=True, backend="hip").to(gpu).eval()
    args = argparse.Namespace(min_depth=1e-3, max_depth=10.0, garg_crop=False, eigen_crop=False)
    H, W, n = 64, 96, 3
    want = E.validate(model, args, E.SyntheticFrames(n, 1, H, W, seed=5), gpu)
    got, count = E.validate_sharded(model, args, E.SyntheticFrames(n, 1, H, W, seed=5), gpu, with_count=True)
    assert count == n
    hw, hg = _hexdict(want), _hexdict(got)
    assert {k: v for k, v in hg.items() if k != "nll"} == {k: v for k, v in hw.items() if k != "nll"}
    outs, gts, bound = [], [], 0.0
    with torch.no_grad():
        for fr in E.SyntheticFrames(n, 1, H, W, seed=5):
            out = model(fr["img"].to(gpu)).cpu().numpy()
            outs.append(out); gts.append(fr["depth"].numpy())
            s, b = R.frame_sums(out[0, 0], out[0, 1], fr["depth"].numpy()[0, 0], R.VARIANCE, 1e-3, 10.0)
            mt, mv = R.margins(out[0, 0], out[0, 1], fr["depth"].numpy()[0, 0], R.VARIANCE, 1e-3, 10.0)
            assert mv > 1e-9, "a variance sits on the clamp: the bound does not hold for it"
            bound += 2.0 * b[12] / s[0] / n
    ref = validate_host(outs, gts, 1e-3, 10.0)
    e_new, e_old = abs(got["nll"] - ref["nll"]), abs(want["nll"] - ref["nll"])
    print(f"nll: restated {ref['nll']:.17g}; sharded off by {e_new:.3e}, validate() off by {e_old:.3e}, bound {bound:.3e}")
    assert e_new <= bound
    assert e_new < e_old


def _run_driver(extra, path):
    cmd = [sys.executable, os.path.join(REPO, "eval_dnet.py"), "--sharded", "--frames", "5", "--batch", "2", "--input_height", "64",
           "--input_width", "96", "--dump_metrics", str(path)] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    return out


def test_eval_dnet_world_2_on_one_gpu_equals_world_1(hip_lib, gpu, tmp_path):
    """python eval_dnet.py --gpus 2 --dist_backend gloo --sharded: two ranks sharing the GPU own 2 batches (4 frames) and 1 batch
    (1 frame); the dumped JSON is the world-1 JSON string for string, and rank 0 alone prints the metric line."""
    one = _run_driver([], tmp_path / "w1.json")
    two = _run_driver(["--gpus", "2", "--dist_backend", "gloo"], tmp_path / "w2.json")
    a, b = (tmp_path / "w1.json").read_text(), (tmp_path / "w2.json").read_text()
    assert a == b
    d = json.loads(a)
    assert d["frames"] == 5 and len(d["metrics"]) == 12
    assert all(math.isfinite(float.fromhex(v)) for v in d["metrics"].values())
    assert one.stdout.count("abs_rel abs_diff") == 1 and two.stdout.count("abs_rel abs_diff") == 1
    assert one.stdout.splitlines()[-1] == two.stdout.splitlines()[-1]
    assert "abs_rel abs_diff" not in two.stderr                # rank 1's output arrives there, tagged: it printed no metric line
