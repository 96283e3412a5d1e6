"""Host side of the sharded, sync-free evaluation: the float64 restatement of the metric kernel and its bounds (tests/metrics_ref.py),
running_average against RunningAverageDict, shard_batches, the argument checks of magnet_depth_metrics_ex, and gather_rows over two
gloo ranks.  No GPU is used."""
import ctypes
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import metrics_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DMIN, DMAX = 1e-3, 10.0
SHAPES = [(1, 1, 1), (1, 1, 5), (3, 7, 13), (2, 64, 96), (1, 129, 128)]          # what tests/test_gpu_metric_table.py runs
KINDS = [R.SIGMA, R.VARIANCE, R.NONE]


def _seed(shape, kind):
    return 1000 * kind + shape[1] * shape[2]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_order_restatement_is_within_the_bounds(shape, kind):
    """The sums added in the kernel's order stay inside the bounds around the fsum form, and the seeded inputs keep every threshold
    and clamp decision more than 1e-9 (relative) away from its edge: the counts are exact."""
    mu, second, gt = R.make_case(*shape, kind, _seed(shape, kind))
    for b in range(shape[0]):
        sec = None if second is None else second[b]
        ref, bound = R.frame_sums(mu[b], sec, gt[b], kind, DMIN, DMAX)
        got = R.frame_sums_kernel_order(mu[b], sec, gt[b], kind, DMIN, DMAX)
        assert np.all(np.abs(got - ref) <= bound), (np.abs(got - ref), bound)
        assert all(got[k] == ref[k] for k in (0, 9, 10, 11))
        mt, mv = R.margins(mu[b], sec, gt[b], kind, DMIN, DMAX)
        assert mt > 1e-9 and mv > 1e-9, (mt, mv)
        assert ref[0] >= 1
        if kind == R.NONE:
            assert got[12] == 0.0 and ref[12] == 0.0


def test_variance_case_has_both_tails():
    _, var, gt = R.make_case(2, 64, 96, R.VARIANCE, _seed((2, 64, 96), R.VARIANCE))
    assert 0.08 < np.mean(var < 1e-6) < 0.12 and 0.08 < np.mean(var > 1.0) < 0.12


@pytest.mark.parametrize("shape", [(3, 7, 13), (2, 64, 96)])
def test_planted_defects_leave_the_bounds(shape):
    """The variance read as sigma (squared once more), and the clamp dropped: both leave the nll bound, and only the nll bound."""
    mu, var, gt = R.make_case(*shape, R.VARIANCE, _seed(shape, R.VARIANCE))
    for b in range(shape[0]):
        ref, bound = R.frame_sums(mu[b], var[b], gt[b], R.VARIANCE, DMIN, DMAX)
        as_sigma = R.frame_sums_kernel_order(mu[b], var[b], gt[b], R.SIGMA, DMIN, DMAX)
        no_clamp = R.frame_sums_kernel_order(mu[b], var[b], gt[b], R.VARIANCE, DMIN, DMAX, clamp=False)
        for bad in (as_sigma, no_clamp):
            assert abs(bad[12] - ref[12]) > bound[12]
            assert np.all(np.abs(bad[:12] - ref[:12]) <= bound[:12])


def test_row_restatement_equals_metrics_from_sums():
    from magnet_amd import metrics as M
    assert R.ROW_ORDER == M.METRIC_ORDER
    mu, second, gt = R.make_case(3, 7, 13, R.SIGMA, 5)
    for b in range(3):
        s = list(R.frame_sums(mu[b], second[b], gt[b], R.SIGMA, DMIN, DMAX)[0]) + [0.0] * 3
        m = M.metrics_from_sums(s)
        assert [float(m[k]).hex() for k in M.METRIC_ORDER] == [v.hex() for v in R.row_from_sums(s, R.SIGMA)]
    empty = R.row_from_sums([0.0] * 16, R.NONE)
    assert all(math.isnan(v) for v in empty[:11]) and empty[11] == 0.0
    assert all(math.isnan(v) for v in R.row_from_sums([0.0] * 16, R.VARIANCE))


def test_running_average_equals_running_average_dict():
    from magnet_amd import evaluate as E, metrics as M
    r = np.random.RandomState(3)
    rows = r.rand(7, 12) * 3.0
    rows[4] = float("nan")                                      # a frame without a valid pixel
    rows[5, 11] = 0.0
    avg = M.RunningAverageDict()
    for row in rows:
        avg.update(dict(zip(M.METRIC_ORDER, [float(v) for v in row])))
    want = avg.get_value()
    for form in (torch.from_numpy(rows), rows.tolist()):
        got = E.running_average(form)
        assert list(got) == list(M.METRIC_ORDER)
        assert [float(got[k]).hex() for k in M.METRIC_ORDER] == [float(want[k]).hex() for k in M.METRIC_ORDER]
    assert all(math.isnan(v) for v in got.values())             # NaN propagates, as in the per-frame loops
    first3 = E.running_average(rows[:3])
    assert all(math.isfinite(v) for v in first3.values())
    assert all(math.isnan(v) for v in E.running_average(torch.zeros(0, 12, dtype=torch.float64)).values())


class _ListLoader:
    def __init__(self, n):
        self.n, self.started = n, 0

    def __len__(self):
        return self.n

    def __iter__(self):
        self.started += 1
        return iter(range(self.n))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_shard_batches_covers_every_batch_once_in_order(n, world):
    from magnet_amd import evaluate as E
    seen = []
    for rank in range(world):
        seen += list(E.shard_batches(_ListLoader(n), rank, world))
    assert seen == list(range(n))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_batches_yields_the_unsharded_stream(world):
    sys.path.insert(0, REPO)
    import eval_dnet
    from magnet_amd import evaluate as E
    whole = list(eval_dnet.SyntheticFrames(5, 2, 8, 12))
    assert len(whole) == 3 and whole[-1]["img"].shape[0] == 1
    got = []
    for rank in range(world):
        got += list(E.shard_batches(eval_dnet.SyntheticFrames(5, 2, 8, 12), rank, world))
    assert len(got) == len(whole)
    for a, b in zip(got, whole):
        assert torch.equal(a["img"], b["img"]) and torch.equal(a["depth"], b["depth"])


def _args(L, **kw):
    a = L.MagnetDepthMetricsArgs()
    a.mu = a.second = a.gt = a.sums = a.rows = a.work = 64
    a.mu_stride = a.second_stride = 40
    a.B, a.H, a.W, a.kind = 2, 4, 5, L.METRICS_SIGMA
    a.min_depth, a.max_depth = 1e-3, 10.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_errors_of_depth_metrics_ex(hip_lib):
    """Every refusal comes back as its code before anything is launched (the pointers here are not device memory)."""
    from magnet_amd import lib as L
    f = hip_lib.magnet_depth_metrics_ex

    def rc(**kw):
        return f(ctypes.byref(_args(L, **kw)), None)

    assert f(None, None) == L.E_NULL
    for name in ("mu", "gt", "work"):
        assert rc(**{name: None}) == L.E_NULL, name
    assert rc(sums=None, rows=None) == L.E_NULL and b"NULL" in hip_lib.magnet_last_error()
    for name in ("B", "H", "W"):
        assert rc(**{name: 0}) == L.E_DIM and rc(**{name: -1}) == L.E_DIM, name
    assert rc(max_depth=1e-3) == L.E_DIM and rc(max_depth=float("nan")) == L.E_DIM
    assert rc(kind=3) == L.E_DIM and rc(kind=-1) == L.E_DIM
    assert rc(second=None) == L.E_DIM                                            # SIGMA without its plane
    assert rc(kind=L.METRICS_VARIANCE, second=None) == L.E_DIM
    assert rc(kind=L.METRICS_NONE) == L.E_DIM                                    # NONE with a plane
    assert rc(H=65536, W=65536) == L.E_DIM                                       # H * W beyond the kernel's 32-bit pixel index
    for win in ((1, 1, 0, 5), (0, 4, 3, 2), (-1, 4, 0, 5), (0, 5, 0, 5), (0, 4, 0, 6), (0, 4, -1, 5)):
        assert rc(crop=1, y0=win[0], y1=win[1], x0=win[2], x1=win[3]) == L.E_DIM, win
    for name in ("sums", "rows", "work"):
        assert rc(**{name: 68}) == L.E_ALIGN, name
    ws = hip_lib.magnet_depth_metrics_workspace
    assert 0 < ws(1) < ws(2) < ws(64) and ws(3) == 3 * ws(1) and ws(1) % 8 == 0
    assert ws(0) == -L.E_DIM and ws(-5) == -L.E_DIM


def test_metric_table_refuses_the_cpu_and_unknown_kinds(hip_lib):
    from magnet_amd import lib as L, metrics as M
    with pytest.raises(L.MagnetError, match="no CPU fallback"):
        M.MetricTable("cpu", DMIN, DMAX)
    with pytest.raises(ValueError, match="unknown kind"):
        M.MetricTable("cuda:0", DMIN, DMAX, kind="std")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rows_of(rank, n):
    return torch.arange(n * 12, dtype=torch.float64).view(n, 12) + 1000.0 * rank + 0.25


def _gather_worker(rank, world, port, q):
    from magnet_amd import dist as mdist, evaluate as E
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    mdist.init_from_env(backend="gloo")
    out = []
    for counts in ((3, 2), (0, 4)):
        rows = _rows_of(rank, counts[rank])
        if counts[rank]:
            rows[-1, 3] = float("nan")                          # a NaN entry travels unchanged
        out.append(E.gather_rows(rows))
    q.put((rank, [o.numpy().tobytes() for o in out], [tuple(o.shape) for o in out], [str(o.dtype) + str(o.device) for o in out]))
    mdist.barrier()
    torch.distributed.destroy_process_group()


def test_gather_rows_two_rank_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for i, counts in enumerate(((3, 2), (0, 4))):
        parts = []
        for rank in range(world):
            rows = _rows_of(rank, counts[rank])
            if counts[rank]:
                rows[-1, 3] = float("nan")
            parts.append(rows)
        want = torch.cat(parts)
        for rank in range(world):
            assert res[rank][2][i] == (sum(counts), 12) and res[rank][3][i] == "torch.float64cpu"
            assert res[rank][1][i] == want.numpy().tobytes(), (i, rank)


def test_gather_rows_without_a_group_is_a_host_copy():
    from magnet_amd import evaluate as E
    rows = _rows_of(0, 3)
    got = E.gather_rows(rows)
    assert got.device.type == "cpu" and torch.equal(got, rows)
