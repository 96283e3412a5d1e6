"""The refinement step with x_d3 read in place by the two fused 3x3 launches (MAGNET.x_d3_source = "auto") against the step that
packs it first ("pack"): bit for bit, eagerly and replayed as a HIP graph.

B = 2, h = 15, w = 32, D = 64, V = 2, I = 1: 1 156 rows, far below the 65 536 from which the library takes the 256-row kernel on its
own, so both stacks are told to take it: ConvStackMFMA.tile_256 = True makes their fused launches pass MAGNET_TILING_BM256, and
x_d3_route() then admits the shape (2 tiles per image under per-image tiling).  lib.entry_log shows which entry points ran."""
import pytest
import torch

from magnet_amd import synth
from tests.parity import to_dev
from tests.stubs import StubDNet, StubFNet, make_args, seeded_magnet_weights

pytestmark = pytest.mark.gpu

B, H, W, D = 2, 15, 32, 64


def _model(gpu, source):
    from magnet_amd.magnet import MAGNET
    m = MAGNET(make_args(D=D, iters=1, dpv_h=H, dpv_w=W), d_net=StubDNet(1), f_net=StubFNet(2, fdim=16))
    seeded_magnet_weights(m, seed=9)
    m = m.to(gpu).eval()
    m.x_d3_source = source
    m.gnet_input_buffer(B, H, W, gpu)
    for st in m._stacks:
        st.tile_256 = True
        st.record_tiles = True
    return m


_CASE = {}


def _case(gpu):
    if not _CASE:
        wl = synth.Workload("t", "scannet", H, W, V=2, D=D, F=16)
        inp = synth.make_inputs(wl, B=B, seed=13)
        x_d3 = (torch.randn(B, 256, H, W, generator=torch.Generator().manual_seed(3)) * 0.5).to(gpu)
        _CASE.update(inp=inp, d=to_dev(inp, gpu), x_d3=x_d3)
    return _CASE["inp"], _CASE["d"], _CASE["x_d3"]


def _refine(m, d, x_d3, inp):
    from magnet_amd import lib
    lib.entry_log = log = []
    try:
        with torch.no_grad():
            out = [p.clone() for p in m.match_and_refine(d["ref_gmms"], x_d3, d["ref_feat"], d["nghbr_feat"], d["nghbr_gmms"], d["nghbr_poses"],
                                                          inp["is_valid"], inp["cam_intrins"], mode="test")]
        torch.cuda.synchronize()
    finally:
        lib.entry_log = None
    return out, log


def test_step_in_place_equals_packed_eager_and_graphed(hip_lib, gpu):
    from magnet_amd.graph import GraphedRefine
    inp, d, x_d3 = _case(gpu)
    res = {}
    for source in ("pack", "auto"):
        m = _model(gpu, source)
        out, log = _refine(m, d, x_d3, inp)
        assert all(st.last_tiles == [(256, 4)] for st in m._stacks), [st.last_tiles for st in m._stacks]   # 2 images x 2 tiles
        g = GraphedRefine(m, d["ref_gmms"], x_d3, d["ref_feat"], d["nghbr_feat"], d["nghbr_gmms"], d["nghbr_poses"], inp["is_valid"],
                          inp["cam_intrins"])
        got = [p.clone() for p in g(*g.static)]
        torch.cuda.synchronize()
        res[source] = (out, log, got)
    (p_out, p_log, p_graph), (a_out, a_log, a_graph) = res["pack"], res["auto"]
    assert "magnet_pack_split" in p_log and "magnet_conv_mfma_nchw" not in p_log
    assert "magnet_pack_split" not in a_log and a_log.count("magnet_conv_mfma_nchw") == 2          # G-Net and the mask head
    assert len(a_out) == 1 and tuple(a_out[0].shape) == (B, 2, 4 * H, 4 * W) and bool(torch.isfinite(a_out[0]).all())
    for name, got in (("auto eager", a_out), ("pack graphed", p_graph), ("auto graphed", a_graph)):
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got, p_out)), name
