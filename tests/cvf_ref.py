"""fp64 reference of est_costvolume_F (the F-Net training volume, reference homography.py:10-75) and of its hand-written
backward, with derived pointwise bounds.  Shared by tests/test_cvf_ref.py (host) and tests/test_gpu_costvolume_f_pointwise.py.

What is fp32 and what is fp64.  The GEOMETRY of this operation is fp32 by contract: the kernels reproduce the reference's
fp32 projection, clamp, floor and tap weights to the bit (warp_math.hpp), and an fp64 geometry would move samples across
texel boundaries.  So the reference takes the geometry from the oracle's dump (oracle.cost_volume_f_geometry: quad origin,
the four fp32 weights and the in-window flag of every (b, v, j, pixel), computed by the same C helper that
oracle.cost_volume_f_raw runs) and does only the ALGEBRA in float64, with w_k the fp32 weights taken as exact numbers:

    cost[b,j,p]           = sum_{v valid, in window} sum_{k<4} sum_f  w_k ref[b,f,p] src_v[f, quad+k] / V
    grad_ref[b,f,p]       = sum_{j, v, k}                             (g[b,j,p] / V) w_k src_v[f, quad+k]
    grad_src_v[f, texel]  = sum_{(j,p,k) -> texel}                    (g[b,j,p] / V) w_k ref[b,f,p]

grad_src is kept in the kernels' padded layout (h+2, w+2): a tap outside the image lands in the one-texel border (the discarded
gradient of the zero padding).  Next to every sum the reference returns S, the sum of the absolute values of its terms, and
n, the number of terms (for cost: 4 F per valid in-window view, the zero-padding taps included; for the gradients: one per
(bin, view, tap) that reaches the element, whatever the value of g).

The bounds (u = 2^-24, gamma(k) = k u / (1 - k u), the standard rounding-error constant).  Every kernel evaluates its sum as
SOME tree of fp32 additions over the terms.  An addition with an exact zero (an empty accumulator, a zeroed buffer, a
zero-padding tap, a filtered G == 0) is exact; every other addition merges the partial sum that holds a given term with at
least one further term, so a term passes through at most n - 1 rounded additions, in any order, association or atomics
interleaving.  The remaining roundings on a term's way are counted from the kernels' code:

  backward (cost_volume_f_bwd.hip, cost_volume_f_gather.hip)
    g / V                          one correctly rounded division                                            1
    (g/V) * w_k                    one product                                                               1
    per-(item, tap) LDS sum        additions (scatter kernels and the grad_ref kernel)                       } together
    accumulation                   one fma per unit: the product G * src (or coef * ref in the gather) is    } <= n - 1
                                   not rounded, the addition is                                              }
    shuffle reduction, hash-table  additions                                                                 }
    cell, flush, global atomics
    G * ref                        one product, in the scatter kernels' grad_src only                        1
  so every element of grad_ref and grad_src, by every route, obeys
    |got - ref| <= gamma(n + C_BWD) S + (n + C_BWD) FLOOR,        C_BWD = 3   (3 products/divisions + (n - 1) additions < n + 3)

  forward, candidate-lane kernel (cost_volume_cand.hip, mode 1)
    dot products                   per tap one fma chain over the lane's channels plus the 8-lane reduction: 4F terms per
                                   view, products unrounded, additions rounded                               } together
    bilerp                         c0 * nw rounded once, then three fmas                                     } <= n - 1 additions
    view sum                       V additions                                                               }
    weight products                one rounding per term (the nw product; the fmas' products are exact)      1
    / V                            one correctly rounded division                                            1
  so   |got - ref| <= gamma(n + C_FWD) S + (n + C_FWD) FLOOR,     C_FWD = 2,   n = 4 F (views in window).
  The generic kernel (path 1, and path 0 where the candidate-lane kernel declines the shape) is bitwise the oracle: ATen's
  order, warp = bilerp(src) first (the nw product rounded, three fmas), then ref * warp rounded, then the channel sum, the
  view sum and the division: weight product 1 + ref product 1 + division 1 + at most n - 1 additions = n + 2 roundings per
  term, so the same bound covers it (tests/test_cvf_ref.py checks the oracle's volume against it); path 1 is compared bit
  for bit besides.

FLOOR = 2^-126 max(1, max|features|): an operation that flushes a denormal operand or result (the hardware's float atomics
may) loses at most 2^-126 absolutely, later scaled by at most one feature value.  With S = 0 (no contribution, or only exact
zeros) the bound is a few 2^-126: such an element must be zero to within denormals — the tests ask for exact zeros there
separately.  Nothing in these bounds is measured from a kernel.

The fp32 emulations (emulate_f32) apply exactly the roundings counted above — g/V, the coefficient product, G * ref for
grad_src, one rounded addition per accumulated term with the fma's product kept exact — in a chosen order of the (view, bin)
chunks and channels, on the CPU; tests/test_cvf_ref.py checks that they stay inside the bounds in forward, reversed and random
order, and that each planted defect (DEFECTS) leaves them.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from magnet_amd import synth
from oracle import oracle

U = 2.0 ** -24
TINY = 2.0 ** -126
C_BWD = 3
C_FWD = 2
SEG = 16                    # texels per gather segment (cvf_gather_src_kernel<16>)
TILE_W, TILE_H = 16, 4      # reference tile of every kernel here
HT_SLOTS = 480              # hash-table slots of cvf_bwd_tile_kernel


def sid_bins(D, dmin=1e-3, dmax=10.0):
    """The reference's SID bin centres (the formula of tests/test_gpu_costvolume_f.py)."""
    return (np.exp(np.log(dmax + 1 - dmin) * (np.arange(D) + 0.5) / D) - (1 - dmin)).astype(np.float32)


def _rot(axis, deg):
    a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
    return {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
            "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]


def _pose(R=None, t=(0.0, 0.0, 0.0)):
    T = np.eye(4, dtype=np.float32)
    if R is not None:
        T[:3, :3] = np.asarray(R, dtype=np.float32)
    T[:3, 3] = t
    return torch.from_numpy(T)


# name -> B, V, h, w, D, F (+ invalid views, explicit poses {(b, v): pose}, bins).  The smallest shapes at which each thing can go
# wrong; what each reaches is asserted from the geometry dump in tests/test_cvf_ref.py::test_coverage.
CASES = {
    "minimum":   dict(B=1, V=1, h=4, w=16, D=1, F=8),
    "ragged":    dict(B=3, V=3, h=9, w=21, D=7, F=24, invalid=[(0, 2)]),
    "seg17":     dict(B=1, V=2, h=5, w=17, D=64, F=64),
    "narrow":    dict(B=2, V=1, h=6, w=7, D=3, F=32),
    "tiles65":   dict(B=1, V=1, h=20, w=208, D=3, F=8, seed=2009),    # a seed whose pose keeps the last tile inside the source image
    "chan72":    dict(B=1, V=2, h=6, w=18, D=5, F=72),
    "chan128":   dict(B=1, V=2, h=6, w=18, D=5, F=128),
    "bins65":    dict(B=1, V=1, h=4, w=16, D=65, F=32),
    "bins256":   dict(B=1, V=1, h=4, w=16, D=256, F=32),
    "views4":    dict(B=1, V=4, h=4, w=16, D=4, F=32),
    "views5":    dict(B=1, V=5, h=4, w=16, D=4, F=32),
    "views29":   dict(B=1, V=29, h=4, w=16, D=4, F=32),
    # rotated poses and forward translation: samples leave the image on every side, fall behind the camera, hit the clamp
    "offimage":  dict(B=2, V=2, h=10, w=22, D=16, F=32,
                      poses={(0, 0): _pose(_rot("y", 25.0), (0.3, -0.2, 0.6)), (0, 1): _pose(_rot("x", -20.0), (-0.1, 0.3, -1.5)),
                             (1, 0): _pose(_rot("z", 30.0), (0.05, 0.4, 1.2)), (1, 1): _pose(_rot("y", -35.0), (-0.4, 0.1, -0.4))}),
    # strong lateral translation and bins uniform in disparity: each pixel's 256 samples sweep the whole row
    "longruns":  dict(B=1, V=1, h=8, w=272, D=256, F=32, poses={(0, 0): _pose(None, (0.5, 0.004, 0.0))},
                      bins=lambda: (1.0 / np.linspace(1.0 / 0.46, 1.0 / 400.0, 256)).astype(np.float32)),
    "wideF":     dict(B=1, V=1, h=4, w=16, D=2, F=160),
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Inputs of one case as CPU tensors / arrays (cached; treat as read-only): synth.make_inputs with a fixed seed, seeded or
    explicit poses, SID bins unless the case names its own, and grad_cost ~ N(0,1) with about 5 % exact zeros and one all-zero bin."""
    c = CASES[name]
    B, V, h, w, D, F = (c[k] for k in "BVhwDF")
    seed = c.get("seed", 1000 + sorted(CASES).index(name))
    wl = synth.Workload("f", "scannet", h, w, V=V, D=D, F=F)
    inp = synth.make_inputs(wl, B=B, seed=seed, invalid=c.get("invalid", ()))
    poses = inp["nghbr_poses"].clone()
    for (b, v), T in c.get("poses", {}).items():
        poses[b, v] = T
    bins = c["bins"]() if "bins" in c else sid_bins(D)
    gen = torch.Generator().manual_seed(seed + 7)
    gout = torch.randn(B, D, h, w, generator=gen)
    gout[torch.rand(B, D, h, w, generator=gen) < 0.05] = 0.0
    if D > 1:
        gout[:, D // 2] = 0.0                                                              # one all-zero bin
    return dict(name=name, B=B, V=V, h=h, w=w, D=D, F=F, ref_feat=inp["ref_feat"], src_feat=inp["nghbr_feat"], poses=poses,
                is_valid=inp["is_valid"], intM=inp["cam_intrins"]["intM"], rays=inp["cam_intrins"]["unit_ray_array_2D"],
                bins=bins, gout=gout)


def oracle_args(case):
    return (case["bins"], case["ref_feat"].numpy(), case["src_feat"].numpy(), case["poses"].numpy(), case["is_valid"].numpy(),
            case["intM"].numpy(), case["rays"].numpy())


@functools.lru_cache(maxsize=None)
def geometry(name):
    c = make_case(name)
    return oracle.cost_volume_f_geometry(c["bins"], c["poses"], c["is_valid"], c["intM"], c["rays"], c["h"], c["w"])


TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))          # (dx, dy) of nw, ne, sw, se

# Planted defects: what a subtly wrong kernel would compute.  Each is applied inside the same fp64 algebra, so the defect is the
# only difference from the reference.
DEFECTS = ("drop_right_tap_at_segment_end", "quad_shift", "missing_1_over_V", "invalid_view_not_skipped", "drop_last_bin",
           "skip_tiles_from_64", "fold_border")


def _terms(case, geo, dtype, defect=None):
    """Yield, per (b, v, j) with contributions, the in-window mask and (padded target index, weight, mask) of the four taps."""
    B, V, h, w, D = (case[k] for k in "BVhwD")
    Wp = w + 2
    ys_, xs_ = np.divmod(np.arange(h * w), w)
    tile = (ys_ // TILE_H) * ((w + TILE_W - 1) // TILE_W) + xs_ // TILE_W
    for b in range(B):
        for v in range(V):
            if not case["is_valid"][b, v] == 1 and defect != "invalid_view_not_skipped":
                continue
            for j in range(D):
                if defect == "drop_last_bin" and j == D - 1 and D > 1:
                    continue
                inw = geo["inwin"][b, v, j].reshape(-1)
                if not inw.any():
                    continue
                x0 = geo["x0"][b, v, j].reshape(-1).astype(np.int64); y0 = geo["y0"][b, v, j].reshape(-1).astype(np.int64)
                if defect == "quad_shift" and j == D // 3 and v == 0:
                    x0 = x0 + 1
                    inw = inw & (x0 < w)
                wts = geo["weights"][b, v, j].reshape(-1, 4)
                taps = []
                for k, (dx, dy) in enumerate(TAPS):
                    px, py = x0 + dx + 1, y0 + dy + 1                                       # padded coordinates
                    ok = inw.copy()
                    if defect == "drop_right_tap_at_segment_end" and dx == 1:
                        ok &= ~(((px - 1) % SEG == 0) & (px - 1 > 0))                       # the right tap opens the next segment
                    if defect == "skip_tiles_from_64":
                        ok &= tile < 64
                    if defect == "fold_border":
                        px, py = np.clip(px, 1, w), np.clip(py, 1, h)
                    idx = np.where(ok, py * Wp + px, 0)
                    taps.append((torch.from_numpy(idx), torch.from_numpy(wts[:, k].astype(np.float64)).to(dtype),
                                 torch.from_numpy(ok)))
                yield b, v, j, torch.from_numpy(inw), taps


def reference(name, defect=None):
    """fp64 cost (B,D,h,w), grad_ref (B,F,h,w), grad_src_pad (V*B,F,h+2,w+2), each as (sum, S, n); n is broadcastable to its sum.
    With `defect`: the same algebra with one planted defect (only the sums are meaningful then)."""
    if defect is None:
        return _reference_cached(name)
    return _reference(name, defect)


@functools.lru_cache(maxsize=None)
def _reference_cached(name):
    return _reference(name, None)


def _reference(name, defect):
    case, geo = make_case(name), geometry(name)
    B, V, h, w, D, F = (case[k] for k in "BVhwDF")
    hw, HWp = h * w, (h + 2) * (w + 2)
    f64 = torch.float64
    ref = case["ref_feat"].to(f64).reshape(B, F, hw)
    srcp = torch.zeros(V * B, F, h + 2, w + 2, dtype=f64)
    srcp[:, :, 1:-1, 1:-1] = case["src_feat"].to(f64)
    srcp = srcp.reshape(V * B, F, HWp)
    g = case["gout"].to(f64).reshape(B, D, hw)
    Vdiv = 1.0 if defect == "missing_1_over_V" else float(V)
    cost = torch.zeros(B, D, hw, dtype=f64); cost_S = torch.zeros_like(cost); cost_n = torch.zeros(B, D, hw, dtype=f64)
    gr = torch.zeros(B, F, hw, dtype=f64); gr_S = torch.zeros_like(gr); gr_n = torch.zeros(B, 1, hw, dtype=f64)
    gs = torch.zeros(V * B, F, HWp, dtype=f64); gs_S = torch.zeros_like(gs); gs_n = torch.zeros(V * B, 1, HWp, dtype=f64)
    for b, v, j, inw, taps in _terms(case, geo, f64, defect):
        s = v * B + b
        for idx, wk, ok in taps:
            okf = ok.to(f64)
            coef = wk * okf                                                                 # (hw)
            sv = srcp[s][:, idx] * coef                                                     # (F, hw): w_k src[f, quad+k]
            cost[b, j] += (ref[b] * sv).sum(0) / Vdiv
            cost_S[b, j] += (ref[b] * sv).abs().sum(0) / Vdiv
            gq = g[b, j] / Vdiv
            gr[b] += gq * sv
            gr_S[b] += (gq * sv).abs()
            gr_n[b, 0] += okf
            gs[s].index_add_(1, idx, (gq * coef) * ref[b])
            gs_S[s].index_add_(1, idx, ((gq * coef) * ref[b]).abs())
            gs_n[s, 0].index_add_(0, idx, okf)
        cost_n[b, j] += 4.0 * F * inw.to(f64)
    sh = lambda t, *shape: t.reshape(*shape)
    return dict(cost=(sh(cost, B, D, h, w), sh(cost_S, B, D, h, w), sh(cost_n, B, D, h, w)),
                grad_ref=(sh(gr, B, F, h, w), sh(gr_S, B, F, h, w), sh(gr_n, B, 1, h, w)),
                grad_src=(sh(gs, V * B, F, h + 2, w + 2), sh(gs_S, V * B, F, h + 2, w + 2), sh(gs_n, V * B, 1, h + 2, w + 2)))


def floor_of(case):
    return TINY * max(1.0, float(case["ref_feat"].abs().max()), float(case["src_feat"].abs().max()))


def _gamma(k):
    return k * U / (1.0 - k * U)


def bound(name, what):
    """The derived pointwise bound of `what` in ('cost', 'grad_ref', 'grad_src'): gamma(n + c) S + (n + c) FLOOR (module docstring)."""
    _, S, n = reference(name)[what]
    k = n + (C_FWD if what == "cost" else C_BWD)
    return _gamma(k) * S + k * floor_of(make_case(name))


def worst(got, name, what, interior_only=False):
    """(max |got - ref| / bound, its index) over every element of `what`; got in the reference's layout (any float dtype).
    interior_only (grad_src): the one-texel border is left out, indices are then those of the (h, w) interior."""
    ref = reference(name)[what][0]
    got = torch.as_tensor(got).to(torch.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ratio = (got - ref).abs() / bound(name, what)
    if interior_only:
        ratio = interior(ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), tuple(int(x) for x in np.unravel_index(i, tuple(ratio.shape)))


def interior(t):
    return t[..., 1:-1, 1:-1]


def _round32(x64):
    return x64.to(torch.float32).to(torch.float64)


def emulate_f32(name, order="forward", seed=0):
    """The kernels' roundings applied on the CPU (module docstring), every fp32 value carried as a float64 that is rounded to fp32
    after each counted operation (an fma is the exact float64 product plus the accumulator, rounded to float64 and then to fp32:
    the double rounding differs from a true fma by at most 2^-53 relative, nothing next to u).  `order` in ('forward', 'reversed', 'random'): the order of the (view, bin) chunks and of the
    channels in the forward's dot products.  Returns dict(cost, grad_ref, grad_src) in the reference's layouts."""
    case, geo = make_case(name), geometry(name)
    B, V, h, w, D, F = (case[k] for k in "BVhwDF")
    hw, HWp = h * w, (h + 2) * (w + 2)
    f64 = torch.float64
    ref = case["ref_feat"].to(f64).reshape(B, F, hw)
    srcp = torch.zeros(V * B, F, h + 2, w + 2, dtype=f64)
    srcp[:, :, 1:-1, 1:-1] = case["src_feat"].to(f64)
    srcp = srcp.reshape(V * B, F, HWp)
    g = case["gout"].to(f64).reshape(B, D, hw)
    chunks = list(_terms(case, geo, f64))
    rng = np.random.default_rng(seed)
    forder = np.arange(F)
    if order == "reversed":
        chunks = chunks[::-1]; forder = forder[::-1].copy()
    elif order == "random":
        chunks = [chunks[i] for i in rng.permutation(len(chunks))]; forder = rng.permutation(F)
    cost = torch.zeros(B, D, hw, dtype=f64)
    gr = torch.zeros(B, F, hw, dtype=f64)
    gs = torch.zeros(V * B, F, HWp, dtype=f64)
    for b, v, j, inw, taps in chunks:
        s = v * B + b
        gq = _round32(g[b, j] / float(V))                                                   # g / V
        c = None
        for k, (idx, wk, ok) in enumerate(taps):
            okf = ok.to(f64)
            sv = srcp[s][:, idx]                                                            # (F, hw)
            dot = torch.zeros(hw, dtype=f64)
            for f in forder:                                                                # fma chain: exact product, rounded sum
                dot = _round32(dot + ref[b, f] * sv[f])
            c = _round32(dot * wk) if k == 0 else _round32(c + dot * wk)                    # bilerp: nw product, then fmas
            coef = _round32(gq * wk) * okf                                                  # (g/V) * w_k
            gr[b] = _round32(gr[b] + coef * sv)                                             # fma per unit
            prod = _round32(coef * ref[b])                                                  # G * ref (scatter kernels)
            sel = torch.nonzero(ok).reshape(-1)
            _scatter_rounded(gs[s], idx[sel], prod[:, sel])
        cost[b, j] = _round32(cost[b, j] + c * inw.to(f64))                                 # view sum
    cost = _round32(cost / float(V))
    return dict(cost=cost.reshape(B, D, h, w), grad_ref=gr.reshape(B, F, h, w), grad_src=gs.reshape(V * B, F, h + 2, w + 2))


def _scatter_rounded(acc, idx, prod):
    """acc[:, idx[p]] += prod[:, p] with one fp32 rounding per addition, duplicates in `idx` included: pixels are applied in rounds
    of distinct targets."""
    if len(idx) == 0:
        return
    order = torch.argsort(idx, stable=True)
    sidx = idx[order]
    first = torch.ones_like(sidx, dtype=torch.bool)
    first[1:] = sidx[1:] != sidx[:-1]
    start = torch.where(first, torch.arange(len(sidx)), torch.zeros_like(sidx))
    rank = torch.arange(len(sidx)) - torch.cummax(start, 0).values                          # position inside the run of equal targets
    for r in range(int(rank.max()) + 1):
        sel = order[rank == r]
        acc[:, idx[sel]] = _round32(acc[:, idx[sel]] + prod[:, sel])
