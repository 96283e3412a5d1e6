"""-m gpu: synchronised BatchNorm on the F-Net's HIP training path (magnet_bn_sync_*, magnet_amd/train_fnet.py).

(a) the four launches in one process, no process group: a grid sharded by images, moments per shard, the records concatenated as
    the all-gather would, merge and apply per shard, against torch.nn.BatchNorm2d in fp64 over the whole grid; the backward likewise.
(b) two ranks over gloo sharing the GPU (one spawn for the module, tests/syncbn_worker.py): a converted PSMNet, forward and backward,
    on 1 + 1 and 2 + 1 images, against a float64 copy of the PSMNet run on the whole batch in one process.
(c) DistributedDataParallel(MAGNET_F(train_backend='hip')) in the same spawn.
(d) the even case over nccl with one GPU per rank (skipped with fewer than two GPUs).
(e) without a process group a converted F-Net gives what the unconverted one gives, bit for bit."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from magnet_amd import fnet, lib
from magnet_amd.magnet import MAGNET_F
from magnet_amd.train_fnet import FNetTrainHIP, fnet_train_hip
from tests import fnet_bwd_ref as R
from tests import syncbn_worker as W

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAN = float("nan")


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- (a) the launches ---------------------------------------------------------------------------------------------------------------
_GRIDS = [((3, 9, 11, 1, 32), (2, 1), True, False, False), ((2, 12, 10, 2, 64), (1, 1), False, True, False),
          ((5, 1, 2, 0, 32), (2, 2, 1), False, True, True), ((2, 1, 1, 0, 32), (1, 1), False, False, False)]


def _shard_rows(split, hp, wp):
    lo = 0
    for n in split:
        yield n, slice(lo * hp * wp, (lo + n) * hp * wp)
        lo += n


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("grid,split,res,relu,f32", _GRIDS)
def test_sync_kernels_forward_vs_torch(hip_lib, gpu, grid, split, res, relu, f32, momentum):
    N, hp, wp, pad, C = grid
    gen = torch.Generator().manual_seed(hp * 31 + C)
    rows, world = N * hp * wp, len(split)
    x = torch.randn(N, hp, wp, C, generator=gen) * 3 + 5
    x[N - split[-1]:] += 100                                                   # the last shard sits 100 away from the others
    bn = torch.nn.BatchNorm2d(C, momentum=momentum).double().train()
    bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(); bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2)
    bn.num_batches_tracked.fill_(2)
    r = torch.randn(rows, C, generator=gen)
    rh = r.to(torch.bfloat16); rl = (r - rh.float()).to(torch.bfloat16)
    ranks = [copy.deepcopy(bn).float().to(gpu) for _ in split]                 # every "rank" owns its module's buffers
    exp = bn(x[:, pad:hp - pad, pad:wp - pad].permute(0, 3, 1, 2).double()).permute(0, 2, 3, 1)
    if res:
        exp = exp + (rh.double() + rl.double()).reshape(N, hp, wp, C)[:, pad:hp - pad, pad:wp - pad]
    if relu:
        exp = exp.clamp_min(0)
    work = torch.empty(lib.BN_BLOCKS * C * 2, dtype=torch.float64, device=gpu)
    xg = torch.full((rows, C + 8), NAN, device=gpu)
    xg[:, :C] = x.reshape(rows, C).to(gpu)                                     # a channel view (x_ld = C + 8)
    records = torch.full((world, 3, C), NAN, dtype=torch.float64, device=gpu)  # what the all-gather leaves on every rank
    for i, (n, sl) in enumerate(_shard_rows(split, hp, wp)):
        lib.bn_sync_moments(xg[sl, :C], (n, hp, wp, pad, C), work, records[i])
    inner = R.interior_mask(N, hp, wp, pad)
    for i, (n, sl) in enumerate(_shard_rows(split, hp, wp)):                   # the record of a shard is that shard's own moments
        xs = x.reshape(rows, C)[sl][inner[sl]].double()
        assert (records[i, 0].cpu() == xs.shape[0]).all()
        np.testing.assert_allclose(records[i, 1].cpu(), xs.mean(0), rtol=1e-12)
        np.testing.assert_allclose(records[i, 2].cpu(), ((xs - xs.mean(0)) ** 2).sum(0), rtol=1e-9, atol=1e-300)
    if grid[1] == 1 and grid[2] == 1:
        assert (records[:, 2] == 0).all()                                      # one value per channel: M2 is exactly zero
    if f32:
        out = torch.full((rows, C), NAN, device=gpu)
    else:
        oh = torch.full((rows, C + 16), 7.0, dtype=torch.bfloat16, device=gpu); ol = oh.clone()
    stats, n_tots = [], []
    for i, (n, sl) in enumerate(_shard_rows(split, hp, wp)):
        m = ranks[i]
        st = torch.full((2, C), NAN, device=gpu)
        n_tot = torch.full((1,), NAN, dtype=torch.float64, device=gpu)
        lib.bn_sync_merge(records, C, st[0], st[1], n_tot, bn.eps, momentum, running_mean=m.running_mean, running_var=m.running_var,
                          num_batches_tracked=m.num_batches_tracked)
        kw = dict(res=(rh.to(gpu)[sl], rl.to(gpu)[sl]) if res else None, relu=relu, stats=False)
        if f32:
            kw["out_f32"] = out[sl]
        else:
            kw["out"] = (oh[sl, 8:8 + C], ol[sl, 8:8 + C])
        lib.bn_train(xg[sl, :C], (n, hp, wp, pad, C), st[0], st[1], work, m.weight.detach(), m.bias.detach(), bn.eps, momentum, **kw)
        stats.append(st); n_tots.append(n_tot)
    if f32:
        got = out.cpu().reshape(N, hp, wp, C)
    else:
        got = (oh.float() + ol.float()).cpu().reshape(N, hp, wp, C + 16)
        assert (got[..., :8] == 14.0).all() and (got[..., 8 + C:] == 14.0).all()           # outside the slice: untouched
        got = got[..., 8:8 + C]
        border = torch.ones(N, hp, wp, dtype=torch.bool); border[:, pad:hp - pad, pad:wp - pad] = False
        assert not got[border].any()
    np.testing.assert_allclose(got[:, pad:hp - pad, pad:wp - pad].numpy(), exp.detach().numpy(), rtol=2e-5, atol=2e-5)
    for i, m in enumerate(ranks):
        assert float(n_tots[i]) == N * (hp - 2 * pad) * (wp - 2 * pad)
        assert torch.equal(stats[i], stats[0])                                 # the same arithmetic on the same bytes
        for name in ("running_mean", "running_var"):
            assert _rel(getattr(m, name), getattr(bn, name)) < 1e-6, name
            assert torch.equal(getattr(m, name), getattr(ranks[0], name)), name
        assert int(m.num_batches_tracked) == 3


@pytest.mark.parametrize("grid,split,res,relu,f32", _GRIDS)
def test_sync_kernels_backward_vs_fp64(hip_lib, gpu, grid, split, res, relu, f32):
    """Per-shard sums, concatenated, apply per shard: dx, and the shards' dgamma / dbeta summed, against fp64 autograd of
    relu(batch_norm(x)) over the whole grid, within the pointwise bounds of tests/fnet_bwd_ref.py (the single-rank test's bars; a
    shard's dgamma / dbeta carry one fp32 store each, so the sum of the shards' bounds bounds their sum)."""
    N, hp, wp, pad, C = grid
    gen = torch.Generator().manual_seed(hp * 37 + C)
    rows, world = N * hp * wp, len(split)
    inner = R.interior_mask(N, hp, wp, pad)
    xv = torch.randn(rows, C, generator=gen) * 3 + 5
    xv[(N - split[-1]) * hp * wp:] += 100
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    xi = xv[inner].double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = torch.nn.functional.batch_norm(xi, None, None, g64, b64, training=True, eps=1e-5)
    mean = xi.detach().mean(0).float()
    invstd = (1.0 / torch.sqrt(xi.detach().var(0, unbiased=False) + 1e-5)).float()
    gv = torch.randn(rows, C, generator=gen) + 0.3 * (xv - mean) * invstd
    (y.clamp_min(0) if relu else y).backward(gv[inner].double())
    xb = torch.full((rows, C + 16), NAN); xb[:, 8:8 + C] = xv; xb[~inner] = NAN           # border rows and other channels: NaN
    gb = torch.full((rows, C + 8), NAN); gb[:, :C] = gv; gb[~inner] = NAN
    xb, gb = xb.to(gpu), gb.to(gpu)
    x, g = xb[:, 8:8 + C], gb[:, :C]
    dev = [t.to(gpu) for t in (mean, invstd, gamma, beta)]
    n_tot = torch.tensor([float(inner.sum())], dtype=torch.float64, device=gpu)
    work = torch.empty((lib.BN_BLOCKS * 2 + 2) * C, dtype=torch.float64, device=gpu)
    sums = torch.full((world, 2, C), NAN, dtype=torch.float64, device=gpu)
    dgamma, dbeta = torch.full((world, C), NAN, device=gpu), torch.full((world, C), NAN, device=gpu)
    bound_g, bound_b = torch.zeros(C, dtype=torch.float64, device=gpu), torch.zeros(C, dtype=torch.float64, device=gpu)
    marginal = 0
    for i, (n, sl) in enumerate(_shard_rows(split, hp, wp)):
        lib.bn_sync_backward_sums(x[sl], (n, hp, wp, pad, C), *dev, relu, g[sl], dgamma[i], dbeta[i], work, sums[i])
        rs = R.bn_backward_ref(x[sl], (n, hp, wp, pad, C), *dev, relu, g[sl])
        R.check(f"dgamma of shard {i}", dgamma[i], *rs["dgamma"])
        R.check(f"dbeta of shard {i}", dbeta[i], *rs["dbeta"])
        assert torch.equal(sums[i, 0].float(), dbeta[i]) and torch.equal(sums[i, 1].float(), dgamma[i])
        bound_g += rs["dgamma"][1]; bound_b += rs["dbeta"][1]
        marginal += rs["marginal"]
    dxh = torch.full((rows, C + 24), 7.0, dtype=torch.bfloat16, device=gpu); dxl = dxh.clone()
    for i, (n, sl) in enumerate(_shard_rows(split, hp, wp)):
        lib.bn_sync_backward_apply(x[sl], (n, hp, wp, pad, C), *dev, relu, g[sl], (dxh[sl, 8:8 + C], dxl[sl, 8:8 + C]), work, sums, n_tot)
    assert (dxh[:, :8] == 7.0).all() and (dxh[:, 8 + C:] == 7.0).all() and (dxl[:, 8 + C:] == 7.0).all()   # outside the slice
    r = R.bn_backward_ref(x, grid, *dev, relu, g)                              # the whole grid, as one rank would have seen it
    got = R.join(dxh[:, 8:8 + C], dxl[:, 8:8 + C])
    worst = max(R.check("dx", got, *r["dx"]), R.check("sum of dgamma", dgamma.double().sum(0), r["dgamma"][0], bound_g),
                R.check("sum of dbeta", dbeta.double().sum(0), r["dbeta"][0], bound_b))
    assert not got[~inner.to(gpu)].any()                                       # border rows are zero
    print(f"sync BN backward {grid} split {split}: worst ratio {worst:.3f} ({marginal} marginal)")
    if marginal == 0:                                                          # no position on the ReLU's edge: autograd's mask is the kernel's
        # fp64 autograd normalises with the unrounded statistics, the kernel (and r) with mean and invstd rounded to fp32 and an xhat
        # of two fp32 operations: |xhat_k - xhat| <= dxh = 3u |xhat| + u |mean| invstd.  That moves dgamma = sum g' xhat by at most
        # eg = sum |g'| dxh, leaves dbeta alone, and moves dx = gs (g' - s1 / n - xhat s2 / n), gs = gamma invstd (one more u), by
        # at most gs (u (|g'| + |s1 / n| + |xhat s2 / n|) + dxh |s2 / n| + |xhat| eg / n).  Added to the kernel's own bounds.
        n = float(n_tot)
        m64, i64 = mean.double(), invstd.double()
        xh = ((xv[inner].double() - m64) * i64).abs()
        gp = gv[inner].double().abs() * ((y.detach() > 0) if relu else 1.0)
        dxh = 3 * R.U * xh + R.U * m64.abs() * i64
        eg = (gp * dxh).sum(0)
        s1, s2 = b64.grad.abs(), g64.grad.abs()
        e_dx = (gamma.double() * i64).abs() * (R.U * (gp + s1 / n + xh * s2 / n) + dxh * s2 / n + xh * eg / n)
        auto, extra = torch.zeros((rows, C), dtype=torch.float64), torch.zeros((rows, C), dtype=torch.float64)
        auto[inner], extra[inner] = xi.grad, 1.01 * e_dx
        R.check("dx vs fp64 autograd", got.cpu(), auto, r["dx"][1].cpu() + extra)
        R.check("sum of dgamma vs fp64 autograd", dgamma.double().sum(0).cpu(), g64.grad, bound_g.cpu() + 1.01 * eg)
        R.check("sum of dbeta vs fp64 autograd", dbeta.double().sum(0).cpu(), b64.grad, bound_b.cpu())


# ---- (b), (c), (d): two ranks ----------------------------------------------------------------------------------------------------
def _spawn(backend, cases, out):
    """Two ranks of tests/syncbn_worker.py, each under `timeout -k 10 300`; the first rank that exits non-zero stops its partner.
    Returns the exit codes and the ranks' stderr."""
    import socket
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))     # as dist.spawn_ranks starts its ranks
        err = open(os.path.join(out, f"{backend}_rank{rank}.err"), "w")
        procs.append((subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "tests", "syncbn_worker.py"),
                                        "--backend", backend, "--out", str(out), "--cases", cases], env=env, stdout=err, stderr=err), err))
    live = set(range(2))
    while live:
        for rank in sorted(live):
            try:
                code = procs[rank][0].wait(timeout=0.25)
            except subprocess.TimeoutExpired:
                continue
            live.discard(rank)
            if code != 0:
                for other in live:
                    procs[other][0].terminate()
    for _, err in procs:
        err.close()
    return [p.returncode for p, _ in procs], [open(os.path.join(out, f"{backend}_rank{r}.err")).read()[-3000:] for r in range(2)]


def _load(out, case):
    return [dict(np.load(os.path.join(out, f"{case}_rank{r}.npz"))) for r in range(2)]


@pytest.fixture(scope="module")
def gloo_run(hip_lib, gpu, tmp_path_factory):
    """The one spawn of the module: both shard cases and the DDP step, two ranks over gloo on the one GPU."""
    out = tmp_path_factory.mktemp("syncbn_gloo")
    codes, errs = _spawn("gloo", "even,uneven,ddp", str(out))
    assert codes == [0, 0], f"exit codes {codes}\n[rank 0]\n{errs[0]}\n[rank 1]\n{errs[1]}"
    return str(out)


_REF = {}


def _whole_batch_reference(case, gpu):
    """The float64 PSMNet on the whole batch in one process (features, buffers, .grad), and the unsharded HIP path's .grad on the
    same batch; computed once per case."""
    if case not in _REF:
        n = sum(W.SHARDS[case])
        img, gfeat = W.images(n), W.feature_gradient(n)
        ref = copy.deepcopy(W.fnet_base()).double().train()
        feat = ref(img.double())
        (feat * gfeat.double()).sum().backward()
        psm = copy.deepcopy(W.fnet_base()).to(gpu).train()
        (fnet_train_hip(FNetTrainHIP(psm), img.to(gpu)) * gfeat.to(gpu)).sum().backward()
        _REF[case] = (feat.detach(), {k: v.detach() for k, v in ref.state_dict().items()},
                      {k: p.grad.detach() for k, p in ref.named_parameters()},
                      {k: p.grad.detach().double().cpu() for k, p in psm.named_parameters()})
    return _REF[case]


@pytest.mark.parametrize("case", ["even", "uneven"])
def test_two_ranks_gloo_vs_fp64_whole_batch(gloo_run, gpu, case):
    feat64, buf64, grad64, grad_hip1 = _whole_batch_reference(case, gpu)
    ranks = _load(gloo_run, case)
    for rank, d in enumerate(ranks):
        lo, hi = W.shard(case, rank)
        errs = [_rel(d["feat"][i], feat64[lo + i]) for i in range(hi - lo)]
        print(f"{case} rank {rank}: features, worst relative L2 per image vs fp64 whole batch {max(errs):.2e}")
        assert max(errs) < 1e-4
        assert bool(d["repeat"]), "a second identical step differed"
    worst = ("", 0.0)
    for k, v in buf64.items():
        if "running" not in k and "num_batches" not in k:
            continue
        a, b = ranks[0]["buf:" + k], ranks[1]["buf:" + k]
        assert a.tobytes() == b.tobytes(), f"{k} differs between the ranks"
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(v) == 101, k
        else:
            worst = max(worst, (k, _rel(a, v)), key=lambda t: t[1])
    print(f"{case}: running statistics, worst relative L2 vs fp64 {worst[1]:.2e} ({worst[0]})")
    assert worst[1] < 1e-4
    errs = {k: (_rel(ranks[0]["grad:" + k].astype(np.float64) + ranks[1]["grad:" + k], g), _rel(grad_hip1[k], g)) for k, g in grad64.items()}
    k, (e2, e1) = max(errs.items(), key=lambda kv: kv[1][0])
    print(f"{case}: sum of the ranks' .grad vs fp64 whole batch: worst {k} {e2:.2e} (unsharded HIP path on the same batch {e1:.2e}; "
          f"its own worst {max(e[1] for e in errs.values()):.2e})")
    assert e2 < 2e-2


def test_ddp_magnet_f(gloo_run, hip_lib, gpu):
    """(c) DDP(MAGNET_F(train_backend='hip')) after convert_sync_batchnorm, B = 1, V = 1 per rank: .grad bit-identical on both ranks and
    half the whole-batch gradient of the one-process torch backend with a float64 F-Net (B = 2; the matching volume and its backward
    are the fp32 HIP kernels in both, the only implementation); one AdamW step leaves the parameters bit-identical."""
    ranks = _load(gloo_run, "ddp")
    keys = [k for k in ranks[0] if k.startswith(("grad:", "param:", "buf:"))]
    assert any(k.startswith("grad:") for k in keys) and any(k.startswith("param:") for k in keys)
    for k in keys:
        assert ranks[0][k].tobytes() == ranks[1][k].tobytes(), f"{k} differs between the ranks"
    case = W.ddp_case()

    class OnHost(torch.nn.Module):
        """The float64 F-Net on the host, its features handed to the GPU."""

        def __init__(self, f_net):
            super().__init__()
            self.f_net = f_net

        def forward(self, imgs):
            return self.f_net(imgs.double().cpu()).to(imgs.device)

    m = MAGNET_F(case[0], OnHost(W.ddp_fnet(case[0]).double()), train_backend="torch").train()
    W.ddp_loss(m, case, 0, 2, gpu).backward()
    errs = {}
    for k, p in m.named_parameters():
        name = "grad:" + k.replace("f_net.f_net.", "f_net.", 1)
        errs[k] = _rel(ranks[0][name], p.grad / 2)
    k, e = max(errs.items(), key=lambda kv: kv[1])
    print(f"DDP step: .grad vs half the fp64 whole-batch gradient: worst {k} {e:.2e}")
    assert e < 2e-2


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: one per nccl rank")
def test_two_ranks_nccl_even(hip_lib, gpu, tmp_path):
    codes, errs = _spawn("nccl", "even", str(tmp_path))
    assert codes == [0, 0], f"exit codes {codes}\n[rank 0]\n{errs[0]}\n[rank 1]\n{errs[1]}"
    feat64, buf64, grad64, _ = _whole_batch_reference("even", gpu)
    ranks = _load(str(tmp_path), "even")
    for rank, d in enumerate(ranks):
        assert _rel(d["feat"][0], feat64[rank]) < 1e-4 and bool(d["repeat"])
    for k in buf64:
        if "running" in k or "num_batches" in k:
            assert ranks[0]["buf:" + k].tobytes() == ranks[1]["buf:" + k].tobytes(), k
    worst = max(_rel(ranks[0]["grad:" + k].astype(np.float64) + ranks[1]["grad:" + k], g) for k, g in grad64.items())
    assert worst < 2e-2


# ---- (e) regression ------------------------------------------------------------------------------------------------------------------
def test_no_group_is_the_single_process_path(hip_lib, gpu):
    """Plain BatchNorm2d, and SyncBatchNorm with no process group: the same features and buffers, bit for bit, at (4, 256, 320)."""
    assert not torch.distributed.is_initialized()
    base = W.fnet_base()
    from tests.stubs import procedural_images
    img = procedural_images(4, 256, 320).to(gpu)
    outs = []
    for convert in (False, True):
        psm = copy.deepcopy(base)
        if convert:
            psm = torch.nn.SyncBatchNorm.convert_sync_batchnorm(psm)
            assert isinstance(psm.firstconv[0][1], torch.nn.SyncBatchNorm)
        psm = psm.to(gpu).train()
        outs.append((FNetTrainHIP(psm).run(img), W.bn_buffers(psm)))
    assert torch.equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k
