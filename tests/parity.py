"""Shared parity helpers for the GPU tests: how a HIP cost volume is compared with the oracle.

The consistency gate |z - mu_w| < kappa*sigma_w (reference homography.py:157-158) is a hard
threshold, so a 1-ulp difference in any upstream quantity can flip a gate and change one cost
entry by a full feature dot product.  Parity is therefore judged as:
  (a) the fraction of entries that differ by more than rounding ("flip candidates") is <= flip_frac,
  (b) everywhere else |hip - oracle| <= atol + rtol*|oracle|,
  (c) downstream, the final-depth abs_rel delta stays < 1e-4 (tests that run the full loop).
"""
import numpy as np
import torch

from oracle import oracle


def to_dev(inp, device):
    out = {}
    for k, v in inp.items():
        if k == "cam_intrins":
            out[k] = v                      # stays on the CPU like the reference's loader hands it over
        elif k == "is_valid":
            out[k] = v
        else:
            out[k] = v.to(device)
    return out


def oracle_cost(inp, k_list, kappa=5.0, d_volume=None, aux=False):
    return oracle.cost_volume_cw(d_volume, inp["ref_gmms"], k_list, inp["ref_feat"], inp["nghbr_feat"],
                                 inp["nghbr_gmms"], inp["nghbr_poses"], inp["is_valid"],
                                 inp["cam_intrins"]["intM"], inp["cam_intrins"]["unit_ray_array_2D"],
                                 kappa, return_aux=aux)


def cost_stats(hip, orc, atol=2e-5, rtol=2e-5):
    hip = hip.detach().cpu().numpy() if isinstance(hip, torch.Tensor) else np.asarray(hip)
    diff = np.abs(hip.astype(np.float64) - orc.astype(np.float64))
    bad = diff > (atol + rtol * np.abs(orc))
    good = ~bad
    return dict(frac_bitwise=float(np.mean(hip == orc)), frac_flip=float(bad.mean()),
                max_abs_nonflip=float(diff[good].max()) if good.any() else 0.0,
                max_abs=float(diff.max()), n=int(diff.size), finite=bool(np.isfinite(hip).all()))


# Tolerances by kernel (include/magnet_hip.h `path`):
#   path 1 (generic gather kernel): every operation mirrors the oracle -> BITWISE equality.
#   path 0/4 (PRODUCTION matcher, cost_volume_fast.hip): tolerance parity — its geometry is not the reference's rounding
#   sequence, so a small fraction of consistency gates flips: gate-flip fraction <= 1e-5, every entry outside
#   the value tolerance must be explained by a flipped gate of one of its views, everything else within 2e-5 + 2e-5*|oracle|.
#   path 2 (exact candidate-lane kernel) and 3 (worklist kernel): gates and sample positions are still exactly the oracle's; the 64-channel
#   sum is re-associated (dot products per tap, then the bilinear combine), so values agree to fp32
#   accumulation noise: |d| <= 2e-5 + 2e-5*|oracle| (costs are O(1..10), sums of 64 products of
#   N(0,1)-scale numbers), and NO entry may differ by more than that (gate flips would).
WORKLIST_ATOL = 2e-5      # measured on MI355X: max |d| 3.8e-6 over all test shapes
WORKLIST_RTOL = 2e-5


GATE_FLIP_FRAC = 1e-5     # SURVEY.md §7 / VERDICT r1: allowed fraction of flipped consistency gates (production matcher)


def flip_scale(h: int, w: int) -> float:
    """The gate-flip RATE of the production contract grows with the matching grid: a gate flips when the kernel's and the reference's
    sample positions fall on different sides of the bilinear (mu, sigma) field's |z - mu| = kappa sigma crossing, and both positions
    carry fp32 rounding of ~ulp(max(h, w)) texels (the same quantity as pos_eps): 1e-5 at grids up to 160 wide (measured 2 - 5e-6 at
    C1 / C2 / C5, 4e-6 at C4 = 304 wide), proportionally more at the full-resolution grids (C2L, 640 wide: measured 1.2e-5 = 4.7x C2)."""
    return max(1.0, (max(h, w) + 1) / 161.0)


def allowed_flips(n_gate: int, scale: float = 1.0) -> int:
    """Flipped gates allowed among n_gate samples at the contract RATE of GATE_FLIP_FRAC.  For the BASELINE shapes (millions of
    gates) that is simply the fraction.  On the small edge-case shapes the expected count is ~1, and a count bound of 1 would fail
    a kernel sitting exactly at the contract rate a third of the time: there the bound is the 99.9 % Poisson quantile of the
    expected count (expected 1.2 -> 6 allowed; 0.02 -> 1)."""
    from scipy.stats import poisson
    lam = GATE_FLIP_FRAC * scale * n_gate
    return int(lam) if lam >= 20 else max(1, int(poisson.ppf(0.999, lam)))


def assert_tolerant_parity(hip, orc, hip_gates=None, orc_gates=None, n_views=4, label="", sens=None, eps=0.0, flip_rate_scale=1.0,
                           inp=None, k_list=None, kappa=5.0, device=None):
    """Production matcher (path 0/4).  With gate bits from both sides (B,V,D,h,w): the gate-flip fraction is <= 1e-5 (at
    least one flip is tolerated on tiny inputs) and every value outside the tolerance sits on an entry with a flipped gate;
    on top of that the fp64 explainer (explain_production: needs the inputs `inp` and `k_list`) checks WHERE the kernel's gates
    disagree with fp64 and the value of every entry, flipped gate or not.
    Without gate bits: the fraction of out-of-tolerance entries is <= n_views * 1e-5.
    Value tolerance: 2e-5 + 2e-5 |oracle| + eps * sens, where sens = position_sensitivity() (the score's slope in the
    sample position) and eps = pos_eps(h, w) texels — see the comment above position_sensitivity()."""
    hipn = hip.detach().cpu().numpy() if isinstance(hip, torch.Tensor) else np.asarray(hip)
    slack = eps * sens if sens is not None else 0.0
    diff0 = np.abs(hipn.astype(np.float64) - orc.astype(np.float64))
    bad0 = diff0 > (WORKLIST_ATOL + WORKLIST_RTOL * np.abs(orc) + slack)
    st = dict(frac_bitwise=float(np.mean(hipn == orc)), frac_flip=float(bad0.mean()),
              max_abs_nonflip=float(diff0[~bad0].max()) if (~bad0).any() else 0.0, max_abs=float(diff0.max()),
              n=int(diff0.size), finite=bool(np.isfinite(hipn).all()),
              frac_over_2e5=float(np.mean(diff0 > WORKLIST_ATOL + WORKLIST_RTOL * np.abs(orc))))
    assert st["finite"] or not np.isfinite(orc).all(), f"{label}: non-finite values in the HIP cost volume"
    if hip_gates is not None:
        hg = hip_gates.detach().cpu().numpy() if isinstance(hip_gates, torch.Tensor) else np.asarray(hip_gates)
        flipped = hg.astype(bool) != orc_gates.astype(bool)                       # (B,V,D,h,w)
        n_flip, n_gate = int(flipped.sum()), int(flipped.size)
        st["gate_flips"], st["gates"], st["gate_flip_frac"] = n_flip, n_gate, n_flip / n_gate
        print(f"[parity {label} production] {st}")
        assert n_flip <= allowed_flips(n_gate, flip_rate_scale), f"{label}: {st} (allowed {allowed_flips(n_gate, flip_rate_scale)})"
        unexplained = bad0 & ~flipped.any(axis=1)
        if unexplained.any():                                                        # show what they are before failing
            idx = np.argwhere(unexplained)[:8]
            for i_ in idx:
                t_ = tuple(i_)
                print(f"[parity {label}] unexplained entry {t_}: hip {hipn[t_]:.7g} oracle {orc[t_]:.7g} |d| {diff0[t_]:.3e} bound "
                      f"{(WORKLIST_ATOL + WORKLIST_RTOL * abs(orc[t_]) + (slack[t_] if sens is not None else 0.0)):.3e} eps*S {(slack[t_] if sens is not None else 0.0):.3e}")
        assert not unexplained.any(), f"{label}: {int(unexplained.sum())} entries differ without a flipped gate: {st}"
        assert inp is not None and k_list is not None, f"{label}: gate bits given without the inputs the fp64 explainer needs"
        ex = assert_explained(inp, k_list, hipn, hg, kappa=kappa, device=device, label=label)
        st.update(explain_gate_ratio=ex["gate_ratio"], explain_residual_ratio=ex["residual_ratio"],
                  explain_gate_disagree=ex["gate_disagree"], explain_gate_marginal=ex["gate_marginal"])
    else:
        print(f"[parity {label} production] {st}")
        assert st["frac_flip"] <= max(n_views * GATE_FLIP_FRAC * flip_rate_scale, 1.5 / st["n"]), f"{label}: {st}"
    return st


def assert_cost_parity(hip, orc, path=0, flip_frac=0.0, label="", n_views=4):
    if path in (0, 4):
        return assert_tolerant_parity(hip, orc, n_views=n_views, label=label)
    if path == 1:
        st = cost_stats(hip, orc, 0.0, 0.0)
        print(f"[parity {label} generic] {st}")
        assert st["finite"] and st["frac_bitwise"] == 1.0, f"{label}: generic kernel not bitwise: {st}"
        return st
    st = cost_stats(hip, orc, WORKLIST_ATOL, WORKLIST_RTOL)
    print(f"[parity {label} fast(path={path})] {st}")
    assert st["finite"], f"{label}: non-finite values in the HIP cost volume"
    assert st["frac_flip"] <= flip_frac, f"{label}: {st}"
    return st


# ---- position-aware value tolerance of the production matcher -------------------------------------------------------
# The production kernel computes the sample position with a different (shorter) rounding sequence than the reference, so
# its texel coordinates differ from the oracle's by a few ulp of the image width.  The score is bilinear in the position
# inside a quad, so such a shift changes an entry by  delta_pos * (|dc/dx| + |dc/dy|)  — for white-noise features (the
# synthetic inputs of SURVEY.md §8d: adjacent texels are independent) that slope is O(10), i.e. a 3e-5 px shift moves the
# score by ~3e-4 although neither side is "wrong".  position_sensitivity() evaluates that slope exactly (fp64 geometry,
# fp64 tap dot products, torch, on the GPU when there is one) so the value tolerance can stay at 2e-5 everywhere else.
def pos_eps(h, w):
    """Allowed position difference in texels: 4 ulp of the padded image extent (reference round trip: ~2 ulp, measured
    1.5e-5 px at w = 160; production kernel: v_rcp_f32 1 ulp + one fused rounding).  The worst case of the two rounding
    chains is ~5 ulp; it shows on the full-resolution stress grids only (C4L, 1216 wide: 2 of 5.5e7 entries at 4.9 ulp): 6 ulp there."""
    return (4.0 if max(h, w) <= 512 else 6.0) * float(np.spacing(np.float32(max(h, w) + 1)))


def position_sensitivity(inp, k_list, gates, device=None):
    """sum_v gate[b,v,j,p] * (|dc/dx| + |dc/dy|) / V  for every cost entry, shape (B,D,h,w), float64 numpy.
    inp: the CPU input dict (features already bf16-rounded if the kernel stores bf16); gates: oracle gate bits (B,V,D,h,w)."""
    dev = device or torch.device("cpu")
    f64 = torch.float64
    ref = inp["ref_feat"].to(dev, f64); src = inp["nghbr_feat"].to(dev, f64)
    B, F, h, w = ref.shape
    V = src.shape[0] // B
    D = len(k_list)
    K = inp["cam_intrins"]["intM"].to(dev, f64); rays = inp["cam_intrins"]["unit_ray_array_2D"].to(dev, f64)
    T = inp["nghbr_poses"].to(dev, f64)
    mu = inp["ref_gmms"][:, 0].reshape(B, 1, h * w).to(dev, f64); sg = inp["ref_gmms"][:, 1].reshape(B, 1, h * w).to(dev, f64)
    kk = torch.tensor([float(np.float32(x)) for x in k_list], dtype=f64, device=dev).reshape(1, D, 1)
    d = mu + sg * kk                                                             # (B,D,hw)
    g = torch.as_tensor(np.asarray(gates), device=dev).reshape(B, V, D, h * w).to(f64)
    out = torch.zeros(B, D, h * w, dtype=f64, device=dev)
    srcp = torch.nn.functional.pad(src, (1, 2, 1, 2))                            # zero border (one extra for the +1 taps)
    for b in range(B):
        rf = ref[b].reshape(F, h * w)                                            # (F,hw)
        for v in range(V):
            if int(inp["is_valid"][b, v]) != 1:
                continue
            R, t = T[b, v, :3, :3], T[b, v, :3, 3]
            rp = (K[b] @ R) @ rays[b]; tp = K[b] @ t                             # (3,hw), (3,)
            P = tp.reshape(3, 1, 1) + rp.reshape(3, 1, h * w) * d[b].reshape(1, D, h * w)
            ix = P[0] / P[2] - 0.5; iy = P[1] / P[2] - 0.5                       # texel coordinates (D,hw)
            ok = torch.isfinite(ix) & torch.isfinite(iy) & (ix >= -1) & (ix < w) & (iy >= -1) & (iy < h)
            x0 = torch.where(ok, torch.floor(ix), torch.zeros_like(ix)); y0 = torch.where(ok, torch.floor(iy), torch.zeros_like(iy))
            fx = torch.where(ok, ix - x0, torch.zeros_like(ix)); fy = torch.where(ok, iy - y0, torch.zeros_like(iy))
            xi = (x0 + 1).long(); yi = (y0 + 1).long()                           # padded coordinates
            sp = srcp[v * B + b]                                                 # (F,h+3,w+3)
            acc = torch.zeros(D, h * w, dtype=f64, device=dev)
            for j0 in range(0, D, 8):                                            # bounded memory: 8 candidates at a time
                sl = slice(j0, min(D, j0 + 8))
                yy, xx = yi[sl], xi[sl]
                c = [torch.einsum("fn,fjn->jn", rf, sp[:, yy + dy, xx + dx]) for dy in (0, 1) for dx in (0, 1)]   # c00 c01 c10 c11
                dcx = (c[1] - c[0]).abs() * (1 - fy[sl]) + (c[3] - c[2]).abs() * fy[sl]
                dcy = (c[2] - c[0]).abs() * (1 - fx[sl]) + (c[3] - c[1]).abs() * fx[sl]
                acc[sl] = (dcx + dcy) * ok[sl]
            out[b] += acc * g[b, v]
    return (out / V).reshape(B, D, h, w).cpu().numpy()


# ---- fp64 explainer of the production matcher's own output ------------------------------------------------------------
# assert_tolerant_parity COUNTS gate flips and value-checks only entries none of whose gates flipped.  explain_production()
# closes both gaps: given the kernel's gate bits, every cost entry has exactly one correct value, (1/V) sum_v gate_hip * dot_v
# (homography.py:116-120,155-159), and every gate bit must agree with the fp64 sign of its margin unless that margin is within
# the position and rounding error the contract allows.
GATE_ROUND_ULPS = 24.0    # coefficient of max|quad corner| in the rounding term r (derivation in explain_production)


def explain_production(inp, k_list, cost, gates, kappa=5.0, device=None, eps=None, label="", max_report=8, fields=False):
    """fp64 explanation of a production-matcher output (cost (B,D,h,w), gates (B,V,D,h,w) = MagnetCostVolumeArgs.gate_bits).

    inp is the CPU input dict the oracle was fed (features bf16-rounded when the kernel stores bf16).  For every (frame, valid
    view, candidate, pixel), in candidate chunks (bounded memory), on the GPU when there is one:
      * candidate depth: the fp32 value the reference forms, sk = sigma * (float)k_j; d = mu + sk (oracle/cost_volume_oracle.c:133);
      * position: homography.py:124-148 in fp64 — P = Kt + (K R ray) d, P /= (P_z + 1e-10), g = (P_xy - c) / c clamped to
        +-10, i = (g + 1) size/2 - 0.5; sampling with grid_sample's zeros padding (one zero texel around the source maps);
      * z = t_z + (R ray)_z d (homography.py:137-138).

    POSITION ERROR.  pos_eps(h, w) texels, scaled per sample by the condition number of the projective divide:
      kappa_P = max(1, (|rp_z d| + |kt_z|) / |P_z|, (|rp_x d| + |kt_x|) / (|P_z| (e + 1)), (|rp_y d| + |kt_y|) / (|P_z| (e + 1))),
    e = max(h, w).  The kernel forms P_c = fma(rp_c, d, kt_c) from fp32 terms that each carry a few roundings (make_pixel_view:
    dot3 of dot3, sgemv-order K t), i.e. an error of a few u (|rp_c d| + |kt_c|); P_x / P_z turns that into a position error of a
    few u |i| when nothing cancels (what pos_eps = 4 - 6 ulp of the extent measures), but kappa_P times more when P_z (or P_x, P_y)
    is the small difference of large terms: samples just in front of the source camera under forward motion (KITTI: z = 0.06 m
    from |t_z| = 1.6 m gives kappa_P ~ 27).  eps_s = pos_eps * kappa_P.

    GATE CHECK.  m = |z - mu_w| - kappa sigma_w; Sm = |dm/dx| + |dm/dy| inside the sample's quad (the slope of m in the sample
    position); every kernel gate bit must equal m < 0 unless |m| <= eps_s * Sm + r.  r bounds what the kernel's fp32
    arithmetic may move m by at a FIXED position (the position difference itself is pos_eps * Sm).  With u = 2^-24 (one
    rounding moves x by <= u|x|) and A_mu, A_sg the largest |corner| of the quad's mu / sigma texels:
      - quad form (elementwise.hip: pack_gmm_quad_kernel, cost_volume_v3.hip gate_view):  q1 = v10 - v00 and q2 = v01 - v00
        round once each (<= u 2A, weight <= 1), q3 = (v11 - v01) - (v10 - v00) three times (<= u (2A + 2A + 4A)), the weight
        bx*by once (<= u |q3| <= 4uA); the three fma round at partial values bounded by A, 3A, A (a bilinear partial sum with
        weights in [-1, 1] summing to 1 at most 3 of them) -> 5uA.  Total 2 + 2 + 8 + 4 + 5 = 21 uA per channel.  The
        interleaved form of cost_volume_fast.hip / cost_volume_fast64.hip (four weight products ax*ay .. and a mul + 3 fma)
        stays below it (2uA weights + 4uA sums = 6uA).  21 is rounded up to GATE_ROUND_ULPS = 24 for the O(u^2) cross terms;
        sigma_w enters multiplied by kappa.
      - z: the kernel's (R ray)_z is an fma dot3 (2 roundings: <= 2u sum_i |R2i ray_i|, times |d|); its candidate depth is
        fma(sigma, k, mu) against the reference's mul-then-add (|d_hip - d| <= u|sk| + 2u|d|, times |(R ray)_z|); zw = fma(...)
        rounds once more (u|z|).
      - the gate itself: the subtraction z - mu_w (u (|z| + |mu_w|)) and the product sigma_w * kappa (u kappa sigma_w).
      r = u (2|z| + |mu_w| + kappa sigma_w + 24 (A_mu + kappa A_sg) + 2 |d| sum_i |R2i ray_i| + |(R ray)_z| (|sk| + 2|d|)).

    VALUE CHECK.  Every entry, flipped gate or not: |cost - (1/V) sum_v gate_hip * dot64_v| <= 2e-5 + 2e-5|c| + S_hip,
    S_hip = (1/V) sum_v gate_hip * eps_s * (|dc/dx| + |dc/dy|) over the views the KERNEL opened (as position_sensitivity()).

    Entries / gates whose fp64 reference is not finite (NaN inputs, degenerate poses) are left to the existing rules.
    Returns dict(gate_ratio = max |m| / bound over the gates that disagree with fp64 (0 if none), residual_ratio = max residual /
    bound, gate_disagree, gate_marginal (disagreeing gates within the bound), gates_checked, entries_checked, and a few
    violating coordinates).  Both ratios must be <= 1.  fields=True adds the per-gate m, Sm, r and the gate bound as (B,V,D,h,w) float64 arrays
    (NaN for invalid views) for the host tests of the model itself."""
    dev = device or (torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
    f64 = torch.float64
    u = 2.0 ** -24
    B, F, h, w = inp["ref_feat"].shape
    V = inp["nghbr_feat"].shape[0] // B
    D = len(k_list)
    hw = h * w
    eps = pos_eps(h, w) if eps is None else eps
    costn = cost.detach().cpu().numpy() if isinstance(cost, torch.Tensor) else np.asarray(cost)
    gn = gates.detach().cpu().numpy() if isinstance(gates, torch.Tensor) else np.asarray(gates)
    cost_t = torch.as_tensor(costn.astype(np.float64), device=dev).reshape(B, D, hw)
    hg = torch.as_tensor(gn.astype(bool), device=dev).reshape(B, V, D, hw)
    # candidate depths exactly as the reference rounds them (fp32 mul, then fp32 add; separate CPU ops, no contraction)
    mu32 = inp["ref_gmms"][:, 0].reshape(B, 1, hw).float(); sg32 = inp["ref_gmms"][:, 1].reshape(B, 1, hw).float()
    k32 = torch.tensor(np.asarray(k_list, dtype=np.float32)).reshape(1, D, 1)
    sk32 = sg32 * k32
    d32 = mu32 + sk32
    dd_all = d32.to(dev, f64); sk_all = sk32.to(dev, f64)
    ref = inp["ref_feat"].to(dev, f64).reshape(B, F, hw)
    srcp = torch.nn.functional.pad(inp["nghbr_feat"].to(dev, f64), (1, 2, 1, 2))           # zeros padding (+1 for the +1 taps)
    gmp = torch.nn.functional.pad(inp["nghbr_gmms"].to(dev, f64), (1, 2, 1, 2))
    K = inp["cam_intrins"]["intM"].to(dev, f64); rays = inp["cam_intrins"]["unit_ray_array_2D"].to(dev, f64)
    T = inp["nghbr_poses"].to(dev, f64)
    Wq = w + 3
    cw, ch = w / 2.0, h / 2.0
    acc = torch.zeros(B, D, hw, dtype=f64, device=dev)
    sen = torch.zeros(B, D, hw, dtype=f64, device=dev)
    n_dis = n_marg = n_gate = 0
    worst_gate = 0.0
    bad_gates = []
    fm = {n_: torch.full((B, V, D, hw), float("nan"), dtype=f64, device=dev) for n_ in ("m", "Sm", "r", "bound")} if fields else None
    J = max(1, min(D, (1 << 21) // max(1, F * hw)))                                         # candidates per chunk
    for b in range(B):
        rf = ref[b]
        for v in range(V):
            if int(inp["is_valid"][b, v]) != 1:
                continue
            R, t = T[b, v, :3, :3], T[b, v, :3, 3]
            rp = (K[b] @ R) @ rays[b]; tp = K[b] @ t                                         # (3,hw), (3,)
            rc = R[2] @ rays[b]; rabs = R[2].abs() @ rays[b].abs()                           # (hw,)
            sp = srcp[v * B + b].reshape(F, -1); gp = gmp[v * B + b].reshape(2, -1)
            for j0 in range(0, D, J):
                sl = slice(j0, min(D, j0 + J))
                dd = dd_all[b, sl]; sk = sk_all[b, sl]                                       # (J,hw)
                P = tp.reshape(3, 1, 1) + rp.reshape(3, 1, hw) * dd.unsqueeze(0)
                zz = P[2] + 1e-10
                den = P[2].abs() * (max(h, w) + 1)
                kap_p = torch.stack([torch.ones_like(zz), (rp[2].abs().reshape(1, hw) * dd.abs() + tp[2].abs()) / P[2].abs(),
                                     (rp[0].abs().reshape(1, hw) * dd.abs() + tp[0].abs()) / den,
                                     (rp[1].abs().reshape(1, hw) * dd.abs() + tp[1].abs()) / den]).amax(0)
                eps_s = eps * torch.nan_to_num(kap_p, nan=1.0, posinf=1.0)           # P_z = 0: no sample (out of range) anyway
                gx = ((P[0] / zz - cw) / cw).clamp(-10.0, 10.0)
                gy = ((P[1] / zz - ch) / ch).clamp(-10.0, 10.0)
                ix = (gx + 1.0) * (w / 2.0) - 0.5; iy = (gy + 1.0) * (h / 2.0) - 0.5
                z = t[2] + rc * dd
                ok = torch.isfinite(ix) & torch.isfinite(iy) & (ix >= -1) & (ix < w) & (iy >= -1) & (iy < h)
                x0 = torch.where(ok, torch.floor(ix), torch.zeros_like(ix)); y0 = torch.where(ok, torch.floor(iy), torch.zeros_like(iy))
                fx = torch.where(ok, ix - x0, torch.zeros_like(ix)); fy = torch.where(ok, iy - y0, torch.zeros_like(iy))
                okf = ok.to(f64)
                base = ((y0 + 1).long() * Wq + (x0 + 1).long()).reshape(-1)
                idx = [base, base + 1, base + Wq, base + Wq + 1]                              # 00 (x0,y0), 01 (x0+1), 10 (y0+1), 11
                shp = dd.shape
                gq = [torch.where(ok, gp[:, i].reshape(2, *shp), torch.zeros((), dtype=f64, device=dev)) for i in idx]
                fx1, fy1 = 1.0 - fx, 1.0 - fy
                mu = gq[0][0] * fx1 * fy1 + gq[1][0] * fx * fy1 + gq[2][0] * fx1 * fy + gq[3][0] * fx * fy
                sg = gq[0][1] * fx1 * fy1 + gq[1][1] * fx * fy1 + gq[2][1] * fx1 * fy + gq[3][1] * fx * fy
                dmux = (gq[1][0] - gq[0][0]) * fy1 + (gq[3][0] - gq[2][0]) * fy
                dmuy = (gq[2][0] - gq[0][0]) * fx1 + (gq[3][0] - gq[1][0]) * fx
                dsgx = (gq[1][1] - gq[0][1]) * fy1 + (gq[3][1] - gq[2][1]) * fy
                dsgy = (gq[2][1] - gq[0][1]) * fx1 + (gq[3][1] - gq[1][1]) * fx
                m = (z - mu).abs() - kappa * sg
                s = torch.sign(z - mu)
                smx = torch.where(s != 0, (s * dmux + kappa * dsgx).abs(), dmux.abs() + kappa * dsgx.abs())
                smy = torch.where(s != 0, (s * dmuy + kappa * dsgy).abs(), dmuy.abs() + kappa * dsgy.abs())
                amu = torch.stack([q[0].abs() for q in gq]).amax(0); asg = torch.stack([q[1].abs() for q in gq]).amax(0)
                r = u * (2 * z.abs() + mu.abs() + kappa * sg.abs() + GATE_ROUND_ULPS * (amu + kappa * asg)
                         + 2 * dd.abs() * rabs + rc.abs() * (sk.abs() + 2 * dd.abs()))
                bound = eps_s * (smx + smy) + r
                if fields:
                    fm["m"][b, v, sl], fm["Sm"][b, v, sl], fm["r"][b, v, sl], fm["bound"][b, v, sl] = m, smx + smy, r, bound
                g = hg[b, v, sl]
                fin = torch.isfinite(m) & torch.isfinite(bound)
                dis = fin & (g != (m < 0))
                n_gate += int(fin.sum())
                if bool(dis.any()):
                    ratio = torch.where(dis, m.abs() / bound, torch.zeros_like(m))
                    n_dis += int(dis.sum()); n_marg += int((dis & (ratio <= 1.0)).sum())
                    worst_gate = max(worst_gate, float(ratio.max()))
                    for jj, pp in torch.nonzero(ratio > 1.0)[:max(0, max_report - len(bad_gates))].tolist():
                        bad_gates.append(dict(frame=b, view=v, cand=j0 + jj, y=pp // w, x=pp % w, gate_hip=int(g[jj, pp]),
                                              m=float(m[jj, pp]), bound=float(bound[jj, pp]), ix=float(ix[jj, pp]), iy=float(iy[jj, pp])))
                # fp64 dot products of the four taps, the bilinear value and its position slope (as position_sensitivity)
                c = []
                for i in idx:
                    tap = sp[:, i].reshape(F, *shp)
                    c.append(torch.where(ok, (rf.unsqueeze(1) * tap).sum(0), torch.zeros((), dtype=f64, device=dev)))
                dot = c[0] * fx1 * fy1 + c[1] * fx * fy1 + c[2] * fx1 * fy + c[3] * fx * fy
                sdot = ((c[1] - c[0]).abs() * fy1 + (c[3] - c[2]).abs() * fy + (c[2] - c[0]).abs() * fx1 + (c[3] - c[1]).abs() * fx) * okf
                acc[b, sl] += torch.where(g, dot, torch.zeros_like(dot))
                sen[b, sl] += torch.where(g, eps_s * sdot, torch.zeros_like(sdot))
    refc = acc / V
    fin = torch.isfinite(refc)
    vbound = WORKLIST_ATOL + WORKLIST_RTOL * refc.abs() + sen / V
    res = (cost_t - refc).abs()
    rr = torch.where(fin, torch.nan_to_num(res / vbound, nan=float("inf")), torch.zeros_like(res))
    worst_res = float(rr.max()) if rr.numel() else 0.0
    bad_entries = []
    for bb, jj, pp in torch.nonzero(rr > 1.0)[:max_report].tolist():
        bad_entries.append(dict(frame=bb, cand=jj, y=pp // w, x=pp % w, cost=float(cost_t[bb, jj, pp]), ref=float(refc[bb, jj, pp]),
                                bound=float(vbound[bb, jj, pp])))
    st = dict(gate_ratio=worst_gate, residual_ratio=worst_res, gate_disagree=n_dis, gate_marginal=n_marg, gates_checked=n_gate,
              entries_checked=int(fin.sum()), bad_gates=bad_gates, bad_entries=bad_entries)
    if fields:
        st.update({n_: a.reshape(B, V, D, h, w).cpu().numpy() for n_, a in fm.items()})
    print(f"[explain {label}] worst gate margin ratio {worst_gate:.3g}, worst residual ratio {worst_res:.3g}; "
          f"{n_dis} of {n_gate} gates disagree with fp64 ({n_marg} marginal)")
    return st


def assert_explained(inp, k_list, cost, gates, kappa=5.0, device=None, eps=None, label=""):
    """explain_production() and its two bars: every gate that disagrees with fp64 is marginal, every entry within its bound."""
    st = explain_production(inp, k_list, cost, gates, kappa=kappa, device=device, eps=eps, label=label)
    for g in st["bad_gates"]:
        print(f"[explain {label}] gate outside its margin: {g}")
    for e in st["bad_entries"]:
        print(f"[explain {label}] entry outside its bound: {e}")
    assert st["gate_ratio"] <= 1.0, f"{label}: {st['gate_disagree'] - st['gate_marginal']} gates disagree with fp64 beyond the margin ({st['bad_gates'][:2]})"
    assert st["residual_ratio"] <= 1.0, f"{label}: entries differ from (1/V) sum gate_hip * dot64 beyond the bound ({st['bad_entries'][:2]})"
    return st
