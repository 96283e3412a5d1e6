"""CPU: the fp64 reference of the F-Net cost volume and its backward (tests/cvf_ref.py) is what it claims to be, on the very cases the
GPU tests use (tests/test_gpu_costvolume_f_pointwise.py): (a) its gradients equal the oracle's double gradients, and the oracle's fp32
volume lies inside the forward bound; (b) S >= |sum| everywhere; (c) fp32 emulations of the kernels' roundings stay inside the
derived bounds in forward, reversed and random order; (d) each planted defect exceeds a bound at one element at least (the element
and the ratio are printed); (e) what every case claims to reach is asserted from the oracle's geometry dump."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import cvf_ref as R

ALL = list(R.CASES)
WHAT = ("cost", "grad_ref", "grad_src")


@pytest.mark.parametrize("name", ALL)
def test_reference_equals_oracle(name):
    """Same geometry, same algebra: the oracle accumulates its gradients in double in pixel order, the reference per (view, bin) with
    index_add_ — they differ by double rounding only (1e-12 of the element's own S)."""
    c = R.make_case(name)
    o_raw, o_gr, o_gs = oracle.cost_volume_f_raw(*R.oracle_args(c), gout=c["gout"].numpy())
    ref = R.reference(name)
    for what, exp in (("grad_ref", torch.from_numpy(o_gr)), ("grad_src", torch.from_numpy(o_gs))):
        got, S, _ = ref[what]
        if what == "grad_src":
            got, S = R.interior(got), R.interior(S)
        assert bool(((got - exp).abs() <= 1e-12 * S + 1e-300).all()), what
    ratio, at = R.worst(o_raw, name, "cost")                          # the oracle's fp32 volume: ATen order, inside the forward bound
    print(f"{name}: oracle fp32 volume / bound = {ratio:.3f} at {at}")
    assert ratio <= 1.0
    # views the reference must skip: exact zeros, no contribution counted
    B = c["B"]
    for b, v in zip(*np.nonzero(c["is_valid"].numpy() != 1)):
        assert not ref["grad_src"][0][v * B + b].any() and not ref["grad_src"][2][v * B + b].any()


@pytest.mark.parametrize("name", ALL)
def test_S_dominates(name):
    for what in WHAT:
        s, S, n = R.reference(name)[what]
        assert bool((S >= s.abs()).all()) and bool((n >= 0).all())
        assert bool(((S == 0) | (n > 0)).all())                       # a term implies a counted contribution
        assert bool((R.bound(name, what) > 0).all())


EMULATED = ["minimum", "ragged", "seg17", "narrow", "chan72", "views5", "offimage"]


@pytest.mark.parametrize("order", ["forward", "reversed", "random"])
@pytest.mark.parametrize("name", EMULATED)
def test_f32_emulation_inside_bound(name, order):
    emu = R.emulate_f32(name, order, seed=11)
    for what in WHAT:
        ratio, at = R.worst(emu[what], name, what)
        print(f"{name} {order} {what}: emulation / bound = {ratio:.3f} at {at}")
        assert ratio <= 1.0, (what, ratio, at)
        assert ratio > 0.0 or not R.reference(name)[what][1].any()   # the emulation does round: the bound is not vacuous


# defect -> (case that can show it, the outputs it must push over their bound)
PLANTED = {
    "drop_right_tap_at_segment_end": ("seg17", ("grad_src",)),
    "quad_shift": ("ragged", WHAT),
    "missing_1_over_V": ("ragged", WHAT),
    "invalid_view_not_skipped": ("ragged", WHAT),
    "drop_last_bin": ("ragged", WHAT),
    "skip_tiles_from_64": ("tiles65", ("grad_src",)),
    "fold_border": ("offimage", ("grad_src",)),
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_exceeds_bound(defect):
    name, outputs = PLANTED[defect]
    bad = R.reference(name, defect=defect)
    for what in outputs:
        ratio, at = R.worst(bad[what][0], name, what, interior_only=what == "grad_src")   # the border is not part of the result
        print(f"{defect} on {name}: {what}{list(at)} is {ratio:.3g} x its bound")
        assert ratio > 1.0, (defect, what, ratio)
    assert set(PLANTED) == set(R.DEFECTS)


def _valid_inwin(name):
    g = R.geometry(name)
    return g, g["inwin"] & g["valid"]


def test_coverage():
    """What the case table of tests/cvf_ref.py says each case reaches, from the shapes and the geometry dump."""
    C = R.CASES
    tiles = lambda c: ((c["w"] + 15) // 16) * ((c["h"] + 3) // 4)
    segs = lambda c: (c["w"] + R.SEG - 1) // R.SEG
    units = lambda c: c["B"] * c["V"] * c["h"] * segs(c)
    hash_route = lambda c: c["F"] % 32 == 0 and c["V"] <= 4          # launch_cvf_bwd: lds_tile = 73168 + 2048 V <= 80 KB
    assert tiles(C["minimum"]) == 1 and C["minimum"]["w"] == R.SEG and C["minimum"]["D"] == 1
    rg = C["ragged"]
    assert len(rg["invalid"]) == 1 and rg["w"] % R.SEG == 5 and units(rg) == 162 and units(rg) % 4 != 0 and not hash_route(rg)
    assert C["seg17"]["w"] % R.SEG == 1 and hash_route(C["seg17"])
    assert C["narrow"]["w"] < R.SEG
    assert C["chan72"]["F"] % 64 == 8 and C["chan72"]["F"] % 32 != 0 and C["chan128"]["F"] // 32 == 4 and hash_route(C["chan128"])
    assert C["bins65"]["D"] == 65 and C["bins256"]["D"] == 256
    assert hash_route(C["views4"]) and not hash_route(C["views5"])
    assert 4 * (C["views29"]["V"] * 512 + 1360) <= 65536 < 4 * ((C["views29"]["V"] + 1) * 512 + 1360)     # the largest V accepted
    assert C["wideF"]["F"] > 128 and hash_route(C["wideF"])
    for name in R.CASES:                                              # every case has contributions and exact-zero gradients
        c = R.make_case(name)
        assert _valid_inwin(name)[1].any(), name
        assert bool((c["gout"] == 0).any()) and (c["D"] == 1 or not c["gout"][:, c["D"] // 2].any())

    # 65 tiles: the second batch of the gather's box scan; tile 64 contributes to interior texels with a non-zero gradient
    c = R.make_case("tiles65")
    assert tiles(C["tiles65"]) == 65
    g, iw = _valid_inwin("tiles65")
    ys, xs = np.divmod(np.arange(c["h"] * c["w"]), c["w"])
    in64 = ((ys // 4) * 13 + xs // 16 == 64).reshape(c["h"], c["w"])
    hit = iw[0, 0] & in64[None] & (c["gout"][0].numpy() != 0) & (g["x0"][0, 0] >= 0) & (g["x0"][0, 0] < c["w"] - 1) \
        & (g["y0"][0, 0] >= 0) & (g["y0"][0, 0] < c["h"] - 1)
    assert hit.any()
    bad = R.reference("tiles65", defect="skip_tiles_from_64")
    assert R.worst(bad["grad_src"][0], "tiles65", "grad_src", interior_only=True)[0] > 1.0

    # off-image: every edge of the window, outside it, behind the camera, clamped
    c = R.make_case("offimage")
    g, iw = _valid_inwin("offimage")
    assert (iw & (g["x0"] == -1)).any() and (iw & (g["x0"] == c["w"] - 1)).any()
    assert (iw & (g["y0"] == -1)).any() and (iw & (g["y0"] == c["h"] - 1)).any()
    assert (~g["inwin"]).any() and (g["Pz"] <= 0).any() and (g["clamp_x"] | g["clamp_y"]).any()

    # long runs: one pixel column (q step) of some 16x4 tile touches more than HT_SLOTS distinct source texels with a non-zero
    # gradient for one view; the hash table (flushed only between q steps) cannot hold them: it must spill to global atomics
    c = R.make_case("longruns")
    g, iw = _valid_inwin("longruns")
    h, w = c["h"], c["w"]
    live = iw[0, 0] & (c["gout"][0].numpy() != 0)
    most = 0
    for ty in range((h + 3) // 4):
        for x in range(w):
            m = live[:, ty * 4:ty * 4 + 4, x]
            qx, qy = g["x0"][0, 0][:, ty * 4:ty * 4 + 4, x][m] + 1, g["y0"][0, 0][:, ty * 4:ty * 4 + 4, x][m] + 1
            tex = np.concatenate([(qy + dy) * (w + 2) + qx + dx for dx, dy in R.TAPS])
            most = max(most, len(np.unique(tex)))
    print(f"longruns: up to {most} distinct texels per (tile, view, pixel column)")
    assert most > R.HT_SLOTS
