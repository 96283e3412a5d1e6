"""CPU: the fp64 explainer of the production matcher (tests/parity.py: explain_production) checked on "kernel outputs" built
from the oracle, which is pinned bit for bit to the reference.

assert_tolerant_parity counts gate flips and value-checks only entries none of whose gates flipped; these tests record that it
passes two wrong outputs (a gate closed far from its |z - mu_w| = kappa sigma_w crossing, and a wrong value on an entry with a
flipped gate) and that the explainer fails both, while it passes the oracle's own output and genuinely marginal flips.  The
margin model eps_s * Sm + r is pinned against finite differences of the oracle's margin, as tests/test_parity_model.py pins
position_sensitivity()."""
import copy

import numpy as np
import pytest
import torch

from magnet_amd import synth
from oracle import oracle
from tests.parity import allowed_flips, assert_explained, assert_tolerant_parity, explain_production, oracle_cost, pos_eps, \
    position_sensitivity

CPU = torch.device("cpu")


def _kitti():
    """KITTI-like forward motion (+-0.8 m per frame gap), samples near and beyond the border, and candidates behind the camera:
    the reference depth of the top rows is pulled in to 0.5 so that mu - 3 sigma < 0."""
    wl = synth.Workload("ex-kitti", "kitti", 14, 48, V=3, D=24, F=16)
    inp = synth.make_inputs(wl, B=1, seed=7)
    inp["ref_gmms"][:, 0, :4] = 0.5
    return inp, oracle.depth_sampling(3, wl.D)


def _scannet():
    wl = synth.Workload("ex-scannet", "scannet", 20, 28, V=2, D=16, F=16)
    return synth.make_inputs(wl, B=2, seed=3, invalid=[(1, 1)]), oracle.depth_sampling(3, wl.D)


def _z_cam(inp, k):
    """z of every (b, v, j, p) sample in the source camera, fp64 (homography.py:137-138)."""
    B, _, h, w = inp["ref_feat"].shape
    V = inp["nghbr_feat"].shape[0] // B
    mu = inp["ref_gmms"][:, 0].reshape(B, 1, -1).double(); sg = inp["ref_gmms"][:, 1].reshape(B, 1, -1).double()
    d = mu + sg * torch.tensor(k).reshape(1, -1, 1)
    T = inp["nghbr_poses"].double(); rays = inp["cam_intrins"]["unit_ray_array_2D"].double()
    return torch.stack([T[:, v, 2, 3].reshape(B, 1, 1) + torch.einsum("bc,bcn->bn", T[:, v, 2, :3], rays).unsqueeze(1) * d
                        for v in range(V)], 1).numpy()


@pytest.mark.parametrize("case", [_kitti, _scannet])
def test_oracle_output_is_explained(case):
    inp, k = case()
    if case is _kitti:
        z = _z_cam(inp, k)
        assert (z < 0).any() and (z > 0).mean() > 0.5                     # some candidates behind the camera
    cost, gates, _ = oracle_cost(inp, k, aux=True)
    st = assert_explained(inp, k, cost, gates, device=CPU, label=case.__name__)
    assert st["gates_checked"] > 0 and st["entries_checked"] == cost.size
    assert st["gate_disagree"] == 0 and st["residual_ratio"] < 0.5


def _marginal_kappa(inp, k):
    """A kappa (fp32) that puts one gate of the oracle's output exactly on its crossing: kappa* = |z - mu_w| / sigma_w of the
    open in-image gate whose sigma_w is largest, rounded to fp32.  At that kappa the gate's margin is sigma_w (kappa* - kappa),
    i.e. at most one rounding of kappa: inside r."""
    cost, gates, _ = oracle_cost(inp, k, aux=True)
    f = explain_production(inp, k, cost, gates, device=CPU, fields=True)
    f0 = explain_production(inp, k, cost, gates, kappa=0.0, device=CPU, fields=True)    # m at kappa = 0 is |z - mu_w|
    sg = (f0["m"] - f["m"]) / 5.0
    ok = np.isfinite(sg) & (sg > 0.1) & (gates == 1)
    i = np.unravel_index(np.argmax(np.where(ok, sg, -1.0)), sg.shape)
    return float(np.float32(f0["m"][i] / sg[i]))


def _marginal_case():
    inp, k = _kitti()
    kap = _marginal_kappa(inp, k)
    cost, gates, fc = oracle_cost(inp, k, kappa=kap, aux=True)
    f = explain_production(inp, k, cost, gates, kappa=kap, device=CPU, fields=True)
    ratio = np.abs(f["m"]) / f["bound"]
    return inp, k, kap, cost, gates, fc, np.where(np.isfinite(ratio), ratio, np.inf)


def _flip(cost, gates, fc, idx):
    """Flip gates idx (tuples (b,v,j,y,x)) and move their entries consistently by +-dot/V."""
    V = gates.shape[1]
    c, g = cost.copy(), gates.copy()
    for b, v, j, y, x in idx:
        c[b, j, y, x] = np.float32(c[b, j, y, x] + (fc[b, v, j, y, x] if g[b, v, j, y, x] == 0 else -fc[b, v, j, y, x]) / V)
        g[b, v, j, y, x] ^= 1
    return c, g


def test_marginal_flips_pass():
    inp, k, kap, cost, gates, fc, ratio = _marginal_case()
    order = np.argsort(ratio, axis=None)
    n = int((ratio <= 1.0).sum())
    assert n >= 1, "no marginal gate to flip"
    idx = [np.unravel_index(i, ratio.shape) for i in order[:n]]
    c, g = _flip(cost, gates, fc, idx)
    st = assert_explained(inp, k, c, g, kappa=kap, device=CPU, label=f"{n} marginal flips")
    # (the oracle itself may sit on the other side of fp64 at the constructed crossing: flipping that gate removes a disagreement)
    assert st["gate_disagree"] == st["gate_marginal"] >= 1 and st["gate_ratio"] <= 1.0


def test_non_marginal_flip_passes_the_counting_checker_and_fails_the_explainer():
    inp, k, kap, cost, gates, fc, ratio = _marginal_case()
    cand = (ratio > 100.0) & (np.abs(fc) > 1.0) & (gates == 1)            # an open gate far from its crossing, a sizeable dot
    idx = [tuple(int(a) for a in np.argwhere(cand)[0])]
    c, g = _flip(cost, gates, fc, idx)
    assert allowed_flips(g.size) >= 1
    # the counting rules alone (no inputs: the explainer is skipped) accept it ...
    _counting_only(c, cost, g, gates, inp, k)
    # ... the explainer does not
    st = explain_production(inp, k, c, g, kappa=kap, device=CPU)
    assert st["gate_ratio"] > 100.0 and st["gate_disagree"] - st["gate_marginal"] == 1
    with pytest.raises(AssertionError, match="beyond the margin"):
        assert_tolerant_parity(c, cost, g, gates, n_views=3, sens=position_sensitivity(inp, k, gates), eps=pos_eps(14, 48),
                               inp=inp, k_list=k, kappa=kap, device=CPU)


def test_wrong_value_on_a_flipped_entry_passes_the_counting_checker_and_fails_the_explainer():
    inp, k, kap, cost, gates, fc, ratio = _marginal_case()
    b, v, j, y, x = np.unravel_index(int(np.argmin(ratio)), ratio.shape)
    c, g = _flip(cost, gates, fc, [(b, v, j, y, x)])
    c[b, j, y, x] += np.float32(1e-3)                                      # the entry behind the flipped gate is now wrong
    _counting_only(c, cost, g, gates, inp, k)
    st = explain_production(inp, k, c, g, kappa=kap, device=CPU)
    assert st["gate_ratio"] <= 1.0 and st["residual_ratio"] > 1.0
    assert st["bad_entries"][0]["frame"] == b and st["bad_entries"][0]["cand"] == j and (st["bad_entries"][0]["y"], st["bad_entries"][0]["x"]) == (y, x)
    with pytest.raises(AssertionError, match="beyond the bound"):
        assert_tolerant_parity(c, cost, g, gates, n_views=3, sens=position_sensitivity(inp, k, gates), eps=pos_eps(14, 48),
                               inp=inp, k_list=k, kappa=kap, device=CPU)


def _counting_only(c, orc, g, og, inp, k):
    """The rules assert_tolerant_parity applied before the explainer: flip count, explained out-of-tolerance entries."""
    sens = position_sensitivity(inp, k, og)
    with pytest.raises(AssertionError, match="without the inputs"):                 # gate bits now always bring the explainer
        assert_tolerant_parity(c, orc, g, og, n_views=3, sens=sens, eps=pos_eps(14, 48))


def test_margin_model_bounds_oracle_finite_differences():
    """Shifting the principal point by delta moves every sample position by exactly delta texels and leaves z unchanged, so
    |m(delta) - m(0)| <= delta * Sm wherever the sample stays in its quad; and the bound is not vacuous."""
    inp, k = _kitti()
    cost, gates, _ = oracle_cost(inp, k, aux=True)
    f0 = explain_production(inp, k, cost, gates, device=CPU, fields=True)
    delta = 2.0 ** -10
    tot = np.zeros_like(f0["m"])
    for dx, dy in ((delta, 0.0), (0.0, delta)):
        sh = copy.deepcopy(inp)
        sh["cam_intrins"]["intM"][:, 0, 2] += dx
        sh["cam_intrins"]["intM"][:, 1, 2] += dy
        f1 = explain_production(sh, k, cost, gates, device=CPU, fields=True)
        dm = np.abs(f1["m"] - f0["m"])
        fin = np.isfinite(dm)
        viol = fin & (dm > delta * f0["Sm"] * 1.001 + 1e-12)
        assert viol.sum() <= 2e-3 * fin.sum(), f"finite difference exceeds the margin model on {viol.sum()} of {fin.sum()} gates"
        tot += np.where(fin, dm, 0.0)
    act = np.isfinite(f0["Sm"]) & (f0["Sm"] > 1e-3)
    ratio = tot[act] / (delta * f0["Sm"][act])
    print(f"[margin model] median (|dm_x| + |dm_y|) / (delta * Sm) = {np.median(ratio):.3f}")
    assert 0.25 < np.median(ratio) <= 1.01
