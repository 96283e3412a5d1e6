"""-m gpu: streaming inference (magnet_amd/sequence.py graph mode, csrc/frame_pool.hip magnet_scatter_frames).  The feature moves data
and replays launches, so every comparison is bit for bit: the scatter kernel against torch indexing and against the gather, and a
SequenceRunner(graph=True) against a SequenceRunner(graph=False) fed the same calls (and against MAGNET.forward on one window)."""
import json
import os

import pytest
import torch

from magnet_amd import fnet, lib, synth
from magnet_amd.magnet import MAGNET
from magnet_amd.sequence import SequenceRunner
from magnet_amd.standin import make_args, make_dnet, seeded_magnet_weights
from tests.stubs import seeded_fnet_state
from tests.test_gpu_sequence import PerImage, PerImageStubDNet, PerImageStubFNet, _Guarded, _same, SENTINEL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "stream_entry_log.json")

# ---- 1. the kernel alone (the gather test's geometry) ----------------------------------------------------------------------------
H, W, N_SLOTS = 5, 7, 6
R = (H + 2) * (W + 2)
TABLE = [4, -1, 0, N_SLOTS, 2]                 # staged frames 0, 2, 4 go to slots 4, 0, 2; frames 1 (-1) and 3 (one past the pool) are skipped
N = len(TABLE)
GROUPS = ("feat", "gmm", "xd3")


def _staged(F, dt, gpu, gmm_guard):
    g = torch.Generator().manual_seed(2000 + F)
    feat = torch.randn((N, H + 2, W + 2, F), generator=g).to(dt).to(gpu)          # seeded borders too: whole frames are copied
    gmm = _Guarded((N, 2, H, W), torch.float32, gmm_guard, gpu)
    gmm.t.copy_(torch.randn((N, 2, H, W), generator=g))
    xhi = torch.randn((N, R, 256), generator=g).to(torch.bfloat16).to(gpu)
    xlo = torch.randn((N, R, 256), generator=g).to(torch.bfloat16).to(gpu)
    return feat, gmm.t, xhi, xlo


def _pool(F, dt, gpu, gmm_guard):
    return {"feat": _Guarded((N_SLOTS, H + 2, W + 2, F), dt, 64, gpu), "gmm": _Guarded((N_SLOTS, 2, H, W), torch.float32, gmm_guard, gpu),
            "xd3_hi": _Guarded((N_SLOTS, R, 256), torch.bfloat16, 64, gpu), "xd3_lo": _Guarded((N_SLOTS, R, 256), torch.bfloat16, 64, gpu)}


@pytest.mark.parametrize("feat_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("F", [16, 64])
def test_scatter_frames_against_torch_indexing(hip_lib, gpu, F, feat_dtype):
    dt = torch.bfloat16 if feat_dtype == "bf16" else torch.float32
    slots = torch.tensor(TABLE, dtype=torch.int32, device=gpu)
    assert (2 * H * W * 4) % 16 == 8                               # a (mu, sigma) frame is 280 bytes: frames alternate between 0 and 8 past a boundary
    # Guards in floats in front of (the staged gmm, the pool's gmm).  The table moves even frames to even slots, so a staged frame sits
    # 4 g0 mod 16 bytes past a boundary and its slot 4 g1 mod 16.  The gather test's choices (3, 5) and (2, 4) give 12 -> 4 and
    # 8 -> 0: source and destination misaligned differently, float by float.  (4, 4): both on a boundary, 17 vectors and a tail of two
    # floats.  (3, 3): both 12 past one, a head of one float, 17 vectors and a tail of one.
    for skip, guards in [(None, (3, 5)), (None, (2, 4)), (None, (4, 4)), (None, (3, 3))] + [(grp, (3, 5)) for grp in GROUPS]:
        feat, gmm, xhi, xlo = _staged(F, dt, gpu, guards[0])
        pool = _pool(F, dt, gpu, guards[1])
        if guards == (2, 4):
            assert gmm[0].data_ptr() % 16 == 8 and pool["gmm"].t[4].data_ptr() % 16 == 0          # misaligned differently
        if guards == (4, 4):
            assert gmm[0].data_ptr() % 16 == pool["gmm"].t[4].data_ptr() % 16 == 0                  # vector body only + float tail
            assert gmm[2].data_ptr() % 16 == pool["gmm"].t[0].data_ptr() % 16 == 0
        if guards == (3, 3):
            assert gmm[0].data_ptr() % 16 == pool["gmm"].t[4].data_ptr() % 16 == 12                 # head of one float, body, tail
        kw = {}
        if skip != "feat":
            kw["feat"] = feat
        if skip != "gmm":
            kw["gmm"] = gmm
        if skip != "xd3":
            kw["xd3"] = (xhi, xlo)
        lib.scatter_frames(slots, pool_feat=pool["feat"].t, pool_gmm=pool["gmm"].t, pool_xd3=(pool["xd3_hi"].t, pool["xd3_lo"].t), **kw)
        torch.cuda.synchronize()
        staged = {"feat": feat, "gmm": gmm, "xd3_hi": xhi, "xd3_lo": xlo}
        for name, dst in pool.items():
            assert dst.guards_intact(), (skip, guards, name)
            if name.startswith(str(skip)):
                assert bool((dst.t == SENTINEL).all()), (skip, name)                                # a group left out: its pool tensor is untouched
                continue
            for j, s in enumerate(TABLE):
                if 0 <= s < N_SLOTS:
                    assert _same(dst.t[s], staged[name][j]), (skip, guards, name, j, s)
            for s in (1, 3, 5):
                assert bool((dst.t[s] == SENTINEL).all()), (skip, guards, name, s)


@pytest.mark.parametrize("feat_dtype", ["fp32", "bf16"])
def test_scatter_then_gather_round_trip(hip_lib, gpu, feat_dtype):
    F = 16
    dt = torch.bfloat16 if feat_dtype == "bf16" else torch.float32
    feat, gmm, xhi, xlo = _staged(F, dt, gpu, 3)
    slots = torch.tensor(TABLE, dtype=torch.int32, device=gpu)
    pool = {"feat": torch.zeros((N_SLOTS, H + 2, W + 2, F), dtype=dt, device=gpu), "gmm": torch.zeros((N_SLOTS, 2, H, W), device=gpu),
            "hi": torch.zeros((N_SLOTS, R, 256), dtype=torch.bfloat16, device=gpu), "lo": torch.zeros((N_SLOTS, R, 256), dtype=torch.bfloat16, device=gpu)}
    lib.scatter_frames(slots, pool_feat=pool["feat"], pool_gmm=pool["gmm"], pool_xd3=(pool["hi"], pool["lo"]), feat=feat, gmm=gmm, xd3=(xhi, xlo))
    # the same table read as B = N windows without views: the gather's reference outputs are the staged frames (zeros where skipped)
    ref_cl = torch.full((N, H, W, F), SENTINEL, dtype=dt, device=gpu)
    ref_gmm = torch.full((N, 2, H, W), SENTINEL, device=gpu)
    gin = tuple(torch.full((N * R, 256), SENTINEL, dtype=torch.bfloat16, device=gpu) for _ in range(2))
    # and as one window with N - 1 views: src_pad carries whole padded frames
    src_pad = torch.full((N - 1, H + 2, W + 2, F), SENTINEL, dtype=dt, device=gpu)
    lib.gather_views(slots, N, 0, pool_feat=pool["feat"], pool_gmm=pool["gmm"], pool_xd3=(pool["hi"], pool["lo"]),
                     ref_cl=ref_cl, ref_gmm=ref_gmm, gin=(gin[0], gin[1], 256, 0))
    lib.gather_views(slots, 1, N - 1, pool_feat=pool["feat"], src_pad=src_pad)
    torch.cuda.synchronize()
    for j, s in enumerate(TABLE):
        kept = 0 <= s < N_SLOTS
        z = lambda t: t if kept else torch.zeros_like(t)
        assert _same(ref_cl[j], z(feat[j][1:-1, 1:-1])) and _same(ref_gmm[j], z(gmm[j])), j
        assert _same(gin[0][j * R:(j + 1) * R], z(xhi[j])) and _same(gin[1][j * R:(j + 1) * R], z(xlo[j])), j
        if j >= 1:
            assert _same(src_pad[j - 1], z(feat[j])), j


# ---- 2. streaming against the eager runner ------------------------------------------------------------------------------------------
T, IMG, CAP = 8, 256, 4
VARIANTS = ("default", "fp16", "stub")


def stream_model(gpu, variant="default"):
    args = make_args(D=5, iters=2, dpv_h=IMG // 4, dpv_w=IMG // 4, fdim=64, V=2)
    if variant == "stub":
        model = MAGNET(args, d_net=PerImageStubDNet(1), f_net=PerImageStubFNet(2, fdim=64), feat_dtype="bf16").to(gpu).eval()
    else:
        args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
        f = fnet.FNET(args)
        seeded_fnet_state(f.f_net, seed=5)
        kw = dict(conv_precision="fp16", fnet_precision="fp16", dnet_precision="fp16", dnet_split_k="auto") if variant == "fp16" else {}
        d = make_dnet(seed=2, enc_seed=3, backend="hip", split_k=kw.get("dnet_split_k", 0), precision=kw.get("dnet_precision", "bf16x3"))
        d.d_net.encoder = PerImage(d.d_net.encoder)                  # the caller's torch encoder: batch-independent, so forward() can be compared
        model = MAGNET(args, d_net=d, f_net=f, feat_dtype="bf16", dnet_backend="hip", **kw).to(gpu).eval()
    seeded_magnet_weights(model, seed=4, gain=0.3)
    return model


def stream_frames(gpu):
    return torch.rand(T, 3, IMG, IMG, generator=torch.Generator().manual_seed(78)).to(gpu)


def stream_step(t, gpu):
    """The causal window of step t >= 1: reference t - 1, views t - 2 (None at t = 1: is_valid 0) and t."""
    refs, nghbrs = [t - 1], [t - 2 if t >= 2 else None, t]
    poses = synth.make_poses("scannet", 1, 2, torch.Generator().manual_seed(600 + t)).to(gpu)
    valid = torch.tensor([[1 if t >= 2 else 0, 1]], dtype=torch.int32)
    return refs, nghbrs, poses, valid, synth.make_intrinsics("scannet", IMG // 4, IMG // 4, 1)


def run_stream(runner, frames, gpu, steps=range(T), **kw):
    """Frame t arrives at step t; from t = 1 on the window centred on t - 1 is refined.  Returns {t: pred_list (copies)}."""
    out = {}
    with torch.no_grad():
        for t in steps:
            assert runner.add([t], frames[t:t + 1]) == 1
            if t >= 1:
                refs, nghbrs, poses, valid, intr = stream_step(t, gpu)
                out[t] = [p.clone() for p in runner.refine(refs, nghbrs, poses, valid, intr, **kw)]
    return out


def _equal(got, ref):
    return len(got) == len(ref) and all(_same(x, y) for x, y in zip(got, ref))


ADD_KEY, REFINE_KEY = ("add", 1, (3, IMG, IMG)), ("refine", 1, 2, "test")


@pytest.mark.parametrize("variant", VARIANTS)
def test_streaming_equals_eager(hip_lib, gpu, variant):
    """With dnet_split_k='auto' the decoder's split factors depend on the batch's tile count (MAGNET's docstring): forward() on the
    3 images of a window runs other factors than add() on one frame, and an image's bits then differ by fp32 summation order.  The
    forward() side of that variant therefore runs the factors the streaming step ran, forced per layer, which is the documented
    condition for bit-equality; both runners run 'auto' itself."""
    m_graph, m_eager, m_fwd = (stream_model(gpu, variant) for _ in range(3))        # the same seeds: three equal models
    frames = stream_frames(gpu)
    graphed, eager = SequenceRunner(m_graph, CAP, graph=True), SequenceRunner(m_eager, CAP)
    got, ref = run_stream(graphed, frames, gpu), run_stream(eager, frames, gpu)
    assert sorted(got) == sorted(ref) == list(range(1, T))
    for t in ref:
        assert len(ref[t]) == 2 and all(bool(torch.isfinite(p).all()) for p in ref[t])
        assert _equal(got[t], ref[t]), t
    assert not _same(ref[1][-1], ref[2][-1]) and not _same(ref[4][-1], ref[5][-1])
    # capacity 4 over 8 frames: the slots were recycled, and the two pools agree
    assert graphed.pool.slots([4, 5, 6, 7]) == eager.pool.slots([4, 5, 6, 7]) and 3 not in graphed.pool
    for a, b in ((graphed.pool.feat, eager.pool.feat), (graphed.pool.gmm, eager.pool.gmm), (graphed.pool.xd3_hi, eager.pool.xd3_hi),
                 (graphed.pool.xd3_lo, eager.pool.xd3_lo)):
        assert _same(a, b) and bool(a.any())
    assert graphed.encoded == eager.encoded == T
    # one capture per key, replays for the rest
    assert graphed.graph_stats == {"captures": {ADD_KEY: 1, REFINE_KEY: 1}, "replays": {ADD_KEY: T - 1, REFINE_KEY: T - 2}}
    assert eager.graph_stats is None
    # step 5 against MAGNET.forward on the same window
    if variant == "fp16":
        used = {name: S for name, _, S in m_eager._dnet.factors_used}
        assert used == {name: S for name, _, S in m_graph._dnet.factors_used} and max(used.values()) > 1
        m_fwd.dnet_split_k = m_fwd._dnet.split_k = used
    refs, nghbrs, poses, valid, intr = stream_step(5, gpu)
    with torch.no_grad():
        fwd = m_fwd(frames[refs], frames[nghbrs], poses, valid, intr, mode="test")
    assert _equal(got[5], fwd)


def test_static_inputs_are_honoured(hip_lib, gpu):
    frames = stream_frames(gpu)
    graphed, eager = SequenceRunner(stream_model(gpu), CAP, graph=True), SequenceRunner(stream_model(gpu), CAP)
    run_stream(graphed, frames, gpu, range(4)); run_stream(eager, frames, gpu, range(4))
    refs, nghbrs, poses, valid, intr = stream_step(3, gpu)
    other = synth.make_poses("scannet", 1, 2, torch.Generator().manual_seed(9)).to(gpu)
    off = valid.clone(); off[0, 1] = 0
    scaled = dict(intr); scaled["intM"] = intr["intM"] * 1.25
    outs = []
    with torch.no_grad():
        for p, v, c in ((poses, valid, intr), (other, valid, intr), (other, off, intr), (other, off, scaled), (poses, valid, intr)):
            got, ref = graphed.refine(refs, nghbrs, p, v, c), eager.refine(refs, nghbrs, p, v, c)
            assert _equal(got, ref)
            outs.append(ref[-1].clone())
    assert not _same(outs[0], outs[1]) and not _same(outs[1], outs[2]) and not _same(outs[2], outs[3]) and _same(outs[0], outs[4])
    assert graphed.graph_stats["captures"][REFINE_KEY] == 1 and graphed.graph_stats["replays"][REFINE_KEY] == 2 + 5


def test_stale_graphs_are_captured_again(hip_lib, gpu):
    frames = stream_frames(gpu)
    m_graph, m_eager = stream_model(gpu), stream_model(gpu)                          # the same seeds: two equal models
    graphed, eager = SequenceRunner(m_graph, CAP, graph=True), SequenceRunner(m_eager, CAP)
    got, ref = run_stream(graphed, frames, gpu, range(3)), run_stream(eager, frames, gpu, range(3))
    assert _equal(got[2], ref[2])
    caps = graphed.graph_stats["captures"]
    assert caps == {ADD_KEY: 1, REFINE_KEY: 1}
    # (a) new g_net weights between two steps
    state = {k: v + 0.01 * torch.randn(v.shape, generator=torch.Generator().manual_seed(11)).to(v) for k, v in m_graph.g_net.state_dict().items()}
    step2 = stream_step(2, gpu)
    with torch.no_grad():
        before = [p.clone() for p in eager.refine(*step2)]
        assert _equal(before, ref[2])
        m_graph.g_net.load_state_dict(state); m_eager.g_net.load_state_dict(state)
        assert not _same(eager.refine(*step2)[-1], before[-1])                       # the weights matter
    got, ref3 = run_stream(graphed, frames, gpu, [3]), run_stream(eager, frames, gpu, [3])
    assert _equal(got[3], ref3[3]) and caps == {ADD_KEY: 1, REFINE_KEY: 2}
    got, ref4 = run_stream(graphed, frames, gpu, [4]), run_stream(eager, frames, gpu, [4])
    assert _equal(got[4], ref4[4]) and caps == {ADD_KEY: 1, REFINE_KEY: 2}
    # (b) an eager forward with B = 2 between two steps displaces MAGNET's workspaces and both backbones' buffers
    refs, nghbrs, poses, valid, intr = stream_step(2, gpu)
    with torch.no_grad():
        for m in (m_graph, m_eager):
            m(frames[[1, 2]], frames[[0, 1, 2, 3]], torch.cat((poses, poses)), torch.ones(2, 2, dtype=torch.int32),
              synth.make_intrinsics("scannet", IMG // 4, IMG // 4, 2), mode="test")
    got, ref5 = run_stream(graphed, frames, gpu, [5]), run_stream(eager, frames, gpu, [5])
    assert _equal(got[5], ref5[5]) and caps == {ADD_KEY: 2, REFINE_KEY: 3}
    # (c) static_outputs=True hands out the graph's own tensors, the default hands out copies
    s6 = run_stream_raw(graphed, frames, gpu, 6, static_outputs=True)
    kept = [p.clone() for p in s6]
    s7 = run_stream_raw(graphed, frames, gpu, 7, static_outputs=True)
    assert [p.data_ptr() for p in s6] == [p.data_ptr() for p in s7]
    ref67 = run_stream(eager, frames, gpu, [6, 7])
    assert _equal(kept, ref67[6]) and _equal(s7, ref67[7]) and not _same(kept[-1], s7[-1])
    refs, nghbrs, poses, valid, intr = stream_step(7, gpu)
    with torch.no_grad():
        c1, c2 = graphed.refine(refs, nghbrs, poses, valid, intr), graphed.refine(refs, nghbrs, poses, valid, intr)
    assert not set(p.data_ptr() for p in c1) & set(p.data_ptr() for p in c2 + s7) and _equal(c1, c2)
    assert caps == {ADD_KEY: 2, REFINE_KEY: 3}


def run_stream_raw(runner, frames, gpu, t, **kw):
    """Step t, returning what refine() returned (no copies)."""
    with torch.no_grad():
        assert runner.add([t], frames[t:t + 1]) == 1
        refs, nghbrs, poses, valid, intr = stream_step(t, gpu)
        return runner.refine(refs, nghbrs, poses, valid, intr, **kw)


def record_entry_log(runner, frames, gpu, steps=range(4)):
    """The entry points every step of an eager runner calls, in order: [[names of step t]]."""
    log = []
    for t in steps:
        lib.entry_log = []
        try:
            run_stream(runner, frames, gpu, [t])
            log.append(list(lib.entry_log))
        finally:
            lib.entry_log = None
    return log


def test_default_is_the_parents(hip_lib, gpu):
    """graph=False: the launches of a step are those of the runner before graph mode existed (tests/golden/stream_entry_log.json,
    recorded from that commit by tests/golden/make_stream_entry_log.py)."""
    runner = SequenceRunner(stream_model(gpu), CAP, graph=False)
    assert runner.graph_stats is None and runner.graph is False
    log = record_entry_log(runner, stream_frames(gpu), gpu)
    want = json.load(open(GOLDEN))
    assert len(want) == 4 and all(len(step) > 50 for step in want) and "magnet_gather_views" in want[1] and "magnet_gather_views" not in want[0]
    assert log == want
    assert not any("magnet_scatter_frames" in step for step in log)


def test_eval_driver_graph_flag_writes_the_same_metrics(hip_lib, gpu, tmp_path, monkeypatch):
    """eval_synthetic.py --reuse_backbones with and without --graph over a folder of 6 frames (4 windows, 2 per call, so add() takes
    several frames at once and the stand-in torch backbones go through pack_features / pack_split in the graph): the same metrics
    file.  --graph without --reuse_backbones is an argument error."""
    import sys
    import PIL  # noqa: F401  (the scene builder needs it; a missing library is a failure here, not a skip)
    import eval_synthetic
    from magnet_amd import sequence
    from tests.test_data_loader import _make_scene
    runners = []

    class Recorded(SequenceRunner):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            runners.append(self)
    monkeypatch.setattr(sequence, "SequenceRunner", Recorded)
    _make_scene(str(tmp_path), "scene0002_00", 6, raw_wh=(96, 64))
    split = tmp_path / "split.txt"
    split.write_text("".join(f"scene0002_00 {i}\n" for i in (1, 2, 3, 4)))
    base = ["eval_synthetic.py", "--dataset_path", str(tmp_path), "--split", str(split), "--V", "2", "--D", "8", "--iters", "2", "--batch", "2",
            "--window_radius", "1", "--input_height", "64", "--input_width", "96", "--sharded"]
    outs = []
    for extra in (["--reuse_backbones", "--pool_frames", "6"], ["--reuse_backbones", "--pool_frames", "6", "--graph"]):
        path = tmp_path / ("metrics%d.json" % len(outs))
        monkeypatch.setattr(sys, "argv", base + ["--dump_metrics", str(path)] + extra)
        eval_synthetic.main()
        outs.append(path.read_text())
    assert '"frames": 4' in outs[0] and "nan" not in outs[0].lower() and outs[0] == outs[1]
    assert [r.graph for r in runners] == [False, True] and runners[1].encoded == 6
    assert sum(runners[1].graph_stats["captures"].values()) >= 2 and runners[0].graph_stats is None
    monkeypatch.setattr(sys, "argv", base + ["--graph"])
    with pytest.raises(SystemExit):
        eval_synthetic.main()
