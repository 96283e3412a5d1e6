"""Host-side logic that needs no GPU: sampling offsets, synthetic generator contracts, the MAGNET
module's interface (constructor fields, state_dict keys), the sharding helper."""
import numpy as np
import pytest
import torch

from magnet_amd import synth
from magnet_amd.magnet import MAGNET, GNET, depth_sampling
from tests.stubs import StubDNet, StubFNet, make_args, seeded_magnet_weights


@pytest.mark.parametrize("D", [5, 16, 64, 128])
def test_depth_sampling_matches_reference(golden, D):
    np.testing.assert_allclose(depth_sampling(3, D), golden[f"G1_k_D{D}"], rtol=0, atol=2e-15)


def test_workload_bytes_match_survey_table():
    # SURVEY.md §8(d) / BASELINE.md §3 table (MB, decimal)
    exp = {"C1": 17.5, "C2": 18.0, "C4": 49.0, "C5": 40.4, "C2L": 288, "C2Lf": 484, "C4L": 784}
    for k, v in exp.items():
        got = synth.WORKLOADS[k].algorithmic_bytes() / 1e6
        assert abs(got - v) / v < 0.01, (k, got, v)


def test_synth_layouts():
    wl = synth.WORKLOADS["C1"]
    inp = synth.make_inputs(wl, B=2, seed=1, invalid=[(0, 1)])
    assert inp["nghbr_feat"].shape == (wl.V * 2, wl.F, wl.h, wl.w)
    assert inp["nghbr_poses"].shape == (2, wl.V, 4, 4) and inp["is_valid"].dtype == torch.int32
    assert inp["is_valid"][0, 1] == 0 and inp["is_valid"].sum() == 2 * wl.V - 1
    rays = inp["cam_intrins"]["unit_ray_array_2D"]
    assert rays.shape == (2, 3, wl.hw) and torch.all(rays[:, 2] == 1)
    # rotation blocks are orthonormal
    R = inp["nghbr_poses"][:, :, :3, :3].double()
    assert torch.allclose(R @ R.transpose(-1, -2), torch.eye(3, dtype=torch.float64).expand_as(R), atol=1e-6)
    # bf16 workloads hand the oracle bf16-representable features
    inp2 = synth.make_inputs(synth.WORKLOADS["C2"], B=1, seed=0)
    f = inp2["ref_feat"]
    assert torch.equal(f, f.to(torch.bfloat16).float())


def test_magnet_module_interface():
    args = make_args(D=5, iters=3, dpv_h=12, dpv_w=16)
    m = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8))
    keys = set(m.state_dict().keys())
    # the reference's checkpoint key names (models/MAGNET.py:108-118)
    for i in (0, 2, 4, 6):
        assert f"g_net.gnet.{i}.weight" in keys and f"mask_head.{i}.weight" in keys
    assert m.g_net.gnet[0].in_channels == 256 + 5 and m.mask_head[6].out_channels == 9 * 16
    assert len(m.k_list) == 5 and not any(p.requires_grad for p in m.d_net.parameters())
    n = sum(p.numel() for p in m.g_net.parameters())
    assert n == 334082                                  # SURVEY.md §8a A6, D=5
    seeded_magnet_weights(m, 3)
    assert isinstance(m.g_net, GNET)


def test_magnet_loads_backbone_checkpoints_like_the_reference(tmp_path):
    """models/MAGNET.py:80-92: the constructor loads args.DNET_ckpt / args.FNET_ckpt into the frozen backbones ({'model': sd}
    or a bare state_dict, 'module.' prefix stripped).  With the modules passed in, a set path is loaded into the passed module;
    an unset path warns (the module is used as passed); a wrong path raises as the reference's torch.load does."""
    args = make_args(D=5, iters=1, dpv_h=12, dpv_w=16)
    src_d, src_f = StubDNet(11), StubFNet(12, fdim=8)
    torch.save({"model": {"module." + k: v for k, v in src_d.state_dict().items()}}, tmp_path / "d.pt")
    torch.save(src_f.state_dict(), tmp_path / "f.pt")
    args.DNET_ckpt, args.FNET_ckpt = str(tmp_path / "d.pt"), str(tmp_path / "f.pt")
    m = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8))
    for got, want in ((m.d_net, src_d), (m.f_net, src_f)):
        for k, v in want.state_dict().items():
            assert torch.equal(got.state_dict()[k], v), k
    assert not any(p.requires_grad for p in list(m.d_net.parameters()) + list(m.f_net.parameters()))
    args.FNET_ckpt = None
    with pytest.warns(UserWarning, match="FNET_ckpt is not set"):
        MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8))
    args.FNET_ckpt = str(tmp_path / "missing.pt")
    with pytest.raises(FileNotFoundError):
        MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8))


def test_magnet_forward_refuses_cpu():
    from magnet_amd import lib
    args = make_args(D=5, iters=1, dpv_h=12, dpv_w=16)
    m = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=8))
    img = torch.rand(1, 3, 48, 64)
    with pytest.raises(lib.MagnetError):
        m(img, torch.rand(2, 3, 48, 64), synth.make_poses("scannet", 1, 2, torch.Generator().manual_seed(0)),
          torch.ones(1, 2, dtype=torch.int32), synth.make_intrinsics("scannet", 12, 16, 1), mode="test")


def test_data_preprocess_matches_reference(golden):
    """G8: relative poses / validity of utils.data_preprocess incl. a NaN reference and a NaN neighbour."""
    from magnet_amd.preprocess import data_preprocess, split_data_array
    exts = golden["G8_exts"]
    data_array = [{"extM": torch.from_numpy(e), "tag": i} for i, e in enumerate(exts)]
    ref, nghbrs, poses, valid = data_preprocess(data_array, 3)
    assert ref["tag"] == 2 and [d["tag"] for d in nghbrs] == [0, 1, 3, 4]          # middle frame is the reference
    assert poses.dtype == torch.float32 and valid.dtype == torch.int32 and not poses.is_cuda
    np.testing.assert_allclose(poses.numpy(), golden["G8_poses"], rtol=0, atol=1e-6)
    assert np.array_equal(valid.numpy(), golden["G8_valid"])
    assert split_data_array(data_array)[0]["tag"] == 2


def test_metrics_from_sums_and_log_format(tmp_path):
    from magnet_amd import metrics as M
    m = M.metrics_from_sums([4, 2.0, 1.0, 0.5, 1.0, 0.04, 0.2, 0.3, 0.16, 3, 4, 4, 2.0, 0, 0, 0])
    assert m["abs_diff"] == 0.5 and m["abs_rel"] == 0.25 and m["rmse"] == 0.5 and m["a1"] == 0.75 and m["nll"] == 0.5
    path = tmp_path / "log.txt"
    M.log_metrics(str(path), m, "first line")
    lines = path.read_text().splitlines()
    assert lines[0] == "first line" and lines[1] == "abs_rel abs_diff sq_rel rmse rmse_log irmse log_10 silog a1 a2 a3 NLL"
    assert len(lines[2].split()) == 12 and lines[2].split()[0] == "0.2500"
    r = M.RunningAverageDict(); r.update({"a": 1.0}); r.update({"a": 3.0})
    assert r.get_value()["a"] == 2.0


def test_cpu_slices_partition_the_cpus():
    from magnet_amd import dist as mdist
    cpus = list(range(3, 3 + 20))
    parts = [mdist.cpu_slice(r, 8, cpus) for r in range(8)]
    assert sorted(c for p in parts for c in p) == cpus and max(map(len, parts)) - min(map(len, parts)) <= 1
    assert all(p == list(range(p[0], p[0] + len(p))) for p in parts)      # contiguous
    assert mdist.cpu_slice(2, 8, [0, 1, 2]) == [0, 1, 2]                  # fewer CPUs than ranks: no pinning
    assert mdist.cpu_slice(0, 1, cpus) == cpus


def test_roofline_bound_label_follows_the_counters():
    """bench.py: `roofline.bound` is what the live counters say (round-4 verdict, item 6) — "hbm" only when the measured traffic runs
    above half the peak rate, the busier issue pipe above 85 %, "latency (...)" below it, and never an assumed "hbm" without counters."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench._bound_label(None, None, 0.9).startswith("unmeasured")
    assert bench._bound_label(None, 5.0e9, 1.0) == "hbm"                                   # 5 GB in 1 ms = 5 TB/s > half of 8 TB/s
    lat = bench._bound_label({"valu_busy": 0.73, "ta_busy": 0.80, "wait_frac": 0.68}, 1.9e9, 0.87)
    assert lat.startswith("latency (vector-memory address unit") and "80%" in lat
    assert bench._bound_label({"valu_busy": 0.91, "ta_busy": 0.5, "wait_frac": 0.2}, 1.0e9, 1.0) == "vector-ALU issue"
    assert bench._bound_label({"valu_busy": 0.5, "ta_busy": 0.9, "wait_frac": 0.2}, None, 1.0).startswith("vector-memory address unit")


def test_bench_dump_outputs_stays_in_budget_and_samples_the_same_frames(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 .npy per output; over the budget every array keeps the same seeded frames (whole slices along
    its first dimension), so two runs with the same arguments write the same positions; below the budget everything is written."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_for_test3", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    preds = [torch.arange(64 * 2 * 6 * 8, dtype=torch.float32).reshape(64, 2, 6, 8) + i for i in range(2)]
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 16 * 2 * 6 * 8 * 4)      # room for 16 of the 64 frames of each array
    assert bench.dump_outputs(preds, str(tmp_path / "a")) == ["pred_0", "pred_1"]
    bench.dump_outputs(preds, str(tmp_path / "b"))
    a0, a1, b0 = (np.load(tmp_path / d / f"pred_{i}.npy") for d, i in (("a", 0), ("a", 1), ("b", 0)))
    assert a0.dtype == np.float32 and a0.shape == (16, 2, 6, 8) and np.array_equal(a0, b0) and np.array_equal(a1, a0 + 1)
    frames = a0[:, 0, 0, 0] / (2 * 6 * 8)
    assert np.array_equal(a0, preds[0].numpy()[frames.astype(int)]) and np.all(np.diff(frames) > 0)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 2 * 16 * 2 * 6 * 8 * 4 + 2 * 256
    bench.dump_outputs({"cost": torch.ones(3, 5, dtype=torch.bfloat16)}, str(tmp_path / "c"))
    assert np.array_equal(np.load(tmp_path / "c" / "cost.npy"), np.ones((3, 5), np.float32))


def test_counter_pass_children_get_a_single_process_environment():
    """Under `torch.distributed.run --nproc-per-node 1` bench.py's rocprofv3 child runs must not inherit the launcher's rendezvous: with
    TORCHELASTIC_USE_AGENT_STORE their own one-rank group would wait for the agent's store until the pass timed out (seen in round 5)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_for_test2", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    env = bench._child_env({"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "LOCAL_WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1",
                            "MASTER_PORT": "29500", "TORCHELASTIC_USE_AGENT_STORE": "True", "TORCHELASTIC_RUN_ID": "x", "GROUP_RANK": "0",
                            "ROLE_RANK": "0", "PATH": "/usr/bin", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "TMPDIR": "/scratch"})
    assert env == {"PATH": "/usr/bin", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "TMPDIR": "/tmp"}


def test_module_checksum_detects_a_single_changed_weight():
    from magnet_amd import dist as mdist
    net = torch.nn.Linear(7, 5)
    a = mdist.module_checksum(net)
    assert a == mdist.module_checksum(net)
    with torch.no_grad():
        net.weight[3, 2] += 1e-3
    assert mdist.module_checksum(net) != a
    assert mdist.broadcast_verified(net) is True                      # no process group: one rank, trivially equal
