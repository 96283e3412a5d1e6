"""-m gpu: every kernel of the F-Net training volume against fp64, pointwise — the mode-1 candidate-lane forward
(cost_volume_cand.hip), the per-item and the LDS-hash scatter backward (cost_volume_f_bwd.hip) and the gather backward
(cost_volume_f_gather.hip), through lib.cost_volume_cw / lib.cost_volume_f_backward.

The reference, the cases and the bounds are tests/cvf_ref.py's: fp32 geometry from the oracle's dump, fp64 algebra, and per element
|got - ref| <= gamma(n + c) S + (n + c) FLOOR with n and S the count and the absolute sum of the element's own terms (derived there,
not measured; tests/test_cvf_ref.py checks the reference, the bounds and the coverage claims on the host).  The generic forward
(path 1) stays bitwise equal to the oracle.

Backward routes.  Always: `gather` (path 0, magnet_cost_volume_f_backward_ws with the workspace it asks for), `scatter` (path 1,
magnet_cost_volume_f_backward: the hash kernel when F % 32 == 0 and V <= 4, else the per-item kernel) and `short_ws` (path 0 with a
workspace one byte short: the _ws entry point's fallback to the scatter kernels).  Only against the dev library
(MAGNET_TEST_DEV_LIB=1): `gather32` (32-texel segments) and `per_item` (the per-item kernel forced).  Which kernel served a scatter
route is read from the hash kernel's counters (stats[1..3]; the other kernels leave them zero) and printed with the route names.

Buffers (the NaN-guard idiom of tests/test_gpu_elementwise_fwd.py): both gradients and the workspace live inside allocations with
guard bands that must stay untouched.  grad_ref starts as NaN and must be fully written.  On the gather route grad_src_pad starts as
NaN: every interior texel must be written (exact zeros in invalid views), every border texel must still be the sentinel.  On the
scatter routes it starts as zeros: the interior is checked pointwise, the border must be finite.

Worst |got - ref| / bound over all cases on an MI355X (every test prints its own; recorded, never used as a tolerance):
    forward, candidate-lane kernel (path 0 / 2)        cost     0.059 (tiles65)
    gather (16-texel segments)                         grad_ref 0.341   grad_src 0.425 (tiles65)
    scatter entry point, per-item kernel               grad_ref 0.341   grad_src 0.434 (tiles65)
    scatter entry point, hash kernel                   grad_ref 0.339   grad_src 0.447 (longruns: 453 066 units spilled)
    short workspace (fallback)                         as the scatter entry point, case by case
    dev library: 32-texel gather                       grad_ref 0.341   grad_src 0.425
    dev library: forced per-item kernel                grad_ref 0.341   grad_src 0.447
An element with a single term has three roundings against a bound of gamma(4) S, so a ratio can reach 0.75 legitimately: the
bounds have no headroom to give away.  No kernel exceeded its bound.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import cvf_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096
NAN_BITS = 0x7FC00000
WS_BYTE = 0xA5


def _guarded(shape, gpu, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=gpu)
    body = buf[GUARD:GUARD + n].view(shape)
    if fill == 0:
        body.zero_()
    return buf, body


def _sentinel(t):
    return t.contiguous().view(torch.int32) == NAN_BITS


def _guards_ok(buf, what):
    assert bool(_sentinel(buf[:GUARD]).all() and _sentinel(buf[-GUARD:]).all()), f"{what}: write outside the buffer"


def _dev_lib():
    from magnet_amd import lib
    return "_dev" in lib.LIB_PATH


def _routes():
    """name -> (path, short workspace).  The dev-only routes exist only in the library that honours dev_flags."""
    r = {"gather": (0, False), "scatter": (1, False), "short_ws": (0, True)}
    if _dev_lib():
        r.update({"gather32": (0x4000, False), "per_item": (0x2001, False)})
    return r


def _hash_expected(case, route):
    """launch_cvf_bwd: the hash kernel takes F % 32 == 0 with lds_tile = 73168 + 2048 V <= 80 KB, unless the dev bit forces the per-item one."""
    return route != "per_item" and case["F"] % 32 == 0 and case["V"] <= 4


def _gather_takes(case):
    """launch_cvf_bwd_ref_only (the gather route's grad_ref): F * 4 / 16 <= 32 chunks."""
    return case["F"] <= 128


class Dev:
    """One case on the device: packed features and geometry tensors."""

    def __init__(self, case, gpu, frame=None):
        from magnet_amd import lib
        B, V = case["B"], case["V"]
        sel = slice(None) if frame is None else slice(frame, frame + 1)
        src_sel = slice(None) if frame is None else [v * B + frame for v in range(V)]
        self.ref_cl = lib.pack_features(case["ref_feat"][sel].contiguous().to(gpu), lib.FEAT_F32, pad=0)
        self.src_pad = lib.pack_features(case["src_feat"][src_sel].contiguous().to(gpu), lib.FEAT_F32, pad=1)
        self.geo = (case["poses"][sel].contiguous().to(gpu), case["is_valid"][sel].int().contiguous().to(gpu),
                    case["intM"][sel].contiguous().to(gpu), case["rays"][sel].contiguous().to(gpu))
        self.bins = [float(v) for v in case["bins"]]
        self.gout = case["gout"][sel].contiguous().to(gpu)
        self.gpu = gpu

    def forward(self, path):
        from magnet_amd import lib
        return lib.cost_volume_cw(self.ref_cl, self.src_pad, None, *self.geo, 0.0, k_list=self.bins, path=path, mode=1)

    def backward(self, path, short_ws=False, src_fill=0, gout=None, stats=None):
        """-> (grad_ref body, grad_src body), guard bands of both gradients and of the workspace already checked."""
        from magnet_amd import lib
        rbuf, gr = _guarded(tuple(self.ref_cl.shape), self.gpu, "nan")
        sbuf, gs = _guarded(tuple(self.src_pad.shape), self.gpu, src_fill)
        held = []

        def workspace(need):                                                               # handed the size the library asks for
            n = need - 1 if short_ws else need
            wsbuf = torch.full((n + 2 * GUARD,), WS_BYTE, dtype=torch.uint8, device=self.gpu)
            held.append((wsbuf, wsbuf[GUARD:GUARD + n]))
            return held[0][1]

        lib.cost_volume_f_backward(self.ref_cl, self.src_pad, *self.geo, self.bins, self.gout if gout is None else gout, path=path,
                                   stats=stats, grad_ref=gr, grad_src=gs, workspace=workspace)
        torch.cuda.synchronize()
        _guards_ok(rbuf, "grad_ref"); _guards_ok(sbuf, "grad_src_pad")
        assert bool(held) == ((path & 0xff) == 0)
        for wsbuf, ws in held:
            assert bool((wsbuf[:GUARD] == WS_BYTE).all() and (wsbuf[-GUARD:] == WS_BYTE).all()), "write outside the workspace"
            if short_ws:
                assert bool((ws == WS_BYTE).all()), "a refused workspace was written"
        return gr, gs


def _check_backward(name, case, route, gr, gs, gather_semantics):
    """Pointwise check of one route's gradients; returns the worst ratios (grad_ref, grad_src interior)."""
    B, V = case["B"], case["V"]
    assert not bool(_sentinel(gr).any()), f"{route}: grad_ref not fully written"
    r_ref, at_ref = R.worst(gr.permute(0, 3, 1, 2).cpu(), name, "grad_ref")
    border = torch.ones(gs.shape[1:3], dtype=torch.bool, device=gs.device)
    border[1:-1, 1:-1] = False
    if gather_semantics:
        assert not bool(_sentinel(gs[:, 1:-1, 1:-1]).any()), f"{route}: an interior texel of grad_src_pad was not stored"
        assert bool(_sentinel(gs[:, border]).all()), f"{route}: the gather wrote the border of grad_src_pad"
    else:
        assert bool(torch.isfinite(gs).all()), f"{route}: non-finite grad_src_pad"
    for b, v in zip(*np.nonzero(case["is_valid"].numpy() != 1)):
        assert not bool(gs[v * B + b, 1:-1, 1:-1].any()), f"{route}: invalid view ({b}, {v}) is not exactly zero"
    gsc = gs.permute(0, 3, 1, 2).cpu()
    r_src, at_src = R.worst(gsc, name, "grad_src", interior_only=True)
    msg = f"{name} {route}: grad_ref {r_ref:.3f} at {at_ref}, grad_src {r_src:.3f} at {at_src}"
    if not gather_semantics:
        ratio = (gsc.double() - R.reference(name)["grad_src"][0]).abs() / R.bound(name, "grad_src")
        ratio[..., 1:-1, 1:-1] = 0
        msg += f", border (not asserted) {float(ratio.max()):.3f}"
    print(msg)
    assert r_ref <= 1.0, (route, "grad_ref", r_ref, at_ref)
    assert r_src <= 1.0, (route, "grad_src", r_src, at_src)
    return r_ref, r_src


@pytest.mark.parametrize("name", list(R.CASES))
def test_pointwise(hip_lib, gpu, name):
    from magnet_amd import lib
    case = R.make_case(name)
    B, V, F = case["B"], case["V"], case["F"]
    dev = Dev(case, gpu)

    # ---- forward: candidate-lane kernel pointwise (path 0 and 2), generic kernel bitwise (path 1) ----
    o_raw = oracle.cost_volume_f_raw(*R.oracle_args(case))
    assert np.array_equal(dev.forward(1).cpu().numpy(), o_raw)
    cand_takes = F <= 128 and 4 * (V * 512 + 3344) <= 65536          # launch_cv_cand: <= 32 chunks of 16 B, its LDS within 64 KB
    for path in (0, 2):
        if path == 2 and not cand_takes:
            with pytest.raises(lib.MagnetError) as ei:
                dev.forward(2)
            assert ei.value.code == lib.E_SHAPE
            print(f"{name} forward path 2: declined (E_SHAPE), path 0 is the generic kernel")
            continue
        ratio, at = R.worst(dev.forward(path).cpu(), name, "cost")
        print(f"{name} forward path {path}: cost {ratio:.3f} at {at}")
        assert ratio <= 1.0, (path, ratio, at)

    # ---- backward: every route the loaded library has ----
    ran = []
    zero = torch.zeros_like(dev.gout)
    for route, (path, short) in _routes().items():
        gather_sem = (path & 0xff) == 0 and not short and _gather_takes(case)
        stats = torch.zeros(4, dtype=torch.int32, device=gpu)
        if route == "per_item" and not _gather_takes(case):            # the per-item kernel has the same 32-chunk limit: forced, it refuses
            with pytest.raises(lib.MagnetError) as ei:
                dev.backward(path)
            assert ei.value.code == lib.E_DIM
            ran.append(f"{route} = refused (E_DIM)")
            continue
        gr, gs = dev.backward(path, short_ws=short, src_fill="nan" if gather_sem else 0, stats=stats)
        _check_backward(name, case, route, gr, gs, gather_sem)
        st = stats.tolist()
        if gather_sem:
            kernel = "gather + per-item grad_ref"
            assert st == [0, 0, 0, 0]
            gr2, gs2 = dev.backward(path, src_fill="nan")                                   # fixed summation order: bit-identical
            assert torch.equal(gr.view(torch.int32), gr2.view(torch.int32)) and torch.equal(gs.view(torch.int32), gs2.view(torch.int32))
        elif _hash_expected(case, route):
            kernel = f"hash kernel (flushed {st[1]}, merged {st[2]}, spilled {st[3]})"
            assert st[1] > 0 and st[2] + st[3] > 0
        else:
            kernel = "per-item kernel"
            assert st == [0, 0, 0, 0]
        # a zero upstream gradient: exact zeros (the gather stores them; the scatter kernels add nothing)
        gr0, gs0 = dev.backward(path, short_ws=short, src_fill="nan" if gather_sem else 0, gout=zero)
        assert not bool(gr0.any()), route
        assert not bool((gs0[:, 1:-1, 1:-1] if gather_sem else gs0).any()), route
        ran.append(f"{route} = {kernel}")
    print(f"{name} routes: " + "; ".join(ran) + ("" if _dev_lib() else "; gather32 and per_item need the dev library: not run"))

    # ---- gather: frame b alone is bit-identical to frame b inside the batch ----
    if B > 1 and _gather_takes(case):
        gr, gs = dev.backward(0, src_fill="nan")
        for b in range(B):
            gr1, gs1 = Dev(case, gpu, frame=b).backward(0, src_fill="nan")
            assert torch.equal(gr1[0].view(torch.int32), gr[b].view(torch.int32)), b
            for v in range(V):
                assert torch.equal(gs1[v].view(torch.int32), gs[v * B + b].view(torch.int32)), (b, v)


def test_long_runs_spill(hip_lib, gpu):
    """The long-runs case overflows the 480-slot table (asserted from the geometry in tests/test_cvf_ref.py::test_coverage): units go
    to global atomics, and the early flush fires — more flushed texels than one flush per (tile, view, slice) can hold."""
    case = R.make_case("longruns")
    dev = Dev(case, gpu)
    stats = torch.zeros(4, dtype=torch.int32, device=gpu)
    dev.backward(1, stats=stats)
    st = stats.tolist()
    tiles = ((case["w"] + 15) // 16) * ((case["h"] + 3) // 4)
    one_flush_each = R.HT_SLOTS * tiles * case["V"] * (case["F"] // 32)
    print(f"longruns hash kernel: flushed {st[1]} texels (one flush each holds <= {one_flush_each}), merged {st[2]}, spilled {st[3]}")
    assert st[3] > 0
    assert st[1] > one_flush_each


@pytest.mark.parametrize("shape", [dict(V=1, F=136), dict(V=30, F=32)])
def test_refused_shapes_leave_outputs_untouched(hip_lib, gpu, shape):
    """F = 136 (neither <= 128 nor a multiple of 32) and V = 30 (the projection table no longer fits 64 KB): E_DIM on both entry points,
    no output element written."""
    from magnet_amd import lib
    V, F = shape["V"], shape["F"]
    h, w, D = 4, 16, 2
    gen = torch.Generator().manual_seed(3)
    ref_cl = torch.randn(1, h, w, F, generator=gen).to(gpu)
    src_pad = torch.randn(V, h + 2, w + 2, F, generator=gen).to(gpu)
    c = R.make_case("minimum")
    geo = (torch.eye(4).repeat(1, V, 1, 1).to(gpu), torch.ones(1, V, dtype=torch.int32, device=gpu), c["intM"].to(gpu), c["rays"].to(gpu))
    gout = torch.randn(1, D, h, w, generator=gen).to(gpu)
    for path in (0, 1):
        rbuf, gr = _guarded(tuple(ref_cl.shape), gpu, "nan")
        sbuf, gs = _guarded(tuple(src_pad.shape), gpu, "nan")
        with pytest.raises(lib.MagnetError) as ei:
            lib.cost_volume_f_backward(ref_cl, src_pad, *geo, [1.0, 2.0], gout, path=path, grad_ref=gr, grad_src=gs)
        torch.cuda.synchronize()
        assert ei.value.code == lib.E_DIM, (path, ei.value)
        assert "V > 29" in str(ei.value) and "F % 32 == 0" in str(ei.value)
        assert bool(_sentinel(rbuf).all() and _sentinel(sbuf).all()), f"path {path}: a refused call wrote an output"


def test_bf16_features_refused(hip_lib, gpu):
    from magnet_amd import lib
    c = R.make_case("minimum")
    dev = Dev(c, gpu)
    with pytest.raises(lib.MagnetError):
        lib.cost_volume_f_backward(dev.ref_cl.bfloat16(), dev.src_pad.bfloat16(), *dev.geo, dev.bins, dev.gout)
