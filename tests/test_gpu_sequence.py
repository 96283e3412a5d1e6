"""-m gpu: sequence inference (magnet_amd/sequence.py, csrc/frame_pool.hip).  The feature only moves data and re-orders calls, so
every comparison is bit for bit: the gather kernel against torch indexing, SequenceRunner.forward against MAGNET.forward on the
same windows, and the evaluation driver with and without --reuse_backbones."""
import sys

import pytest
import torch
import torch.nn as nn

from magnet_amd import fnet, lib, synth
from magnet_amd.homography import CostVolumeCW
from magnet_amd.magnet import MAGNET
from magnet_amd.sequence import FramePool, SequenceRunner
from magnet_amd.standin import StubDNet, StubFNet, make_args, make_dnet, seeded_magnet_weights
from tests.stubs import seeded_fnet_state
from tests.test_data_loader import _make_scene

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------------------
H, W, B, V, N_SLOTS, GIN_LD, C_OFF = 5, 7, 3, 2, 6, 320, 64
R = (H + 2) * (W + 2)
# [b] = reference of window b, [B + v B + b] = view v of window b.  Slot 2 is used three times; slot 4 is the reference of window 1 and
# view 0 of window 2; window 1 has no view 0 (-1); view 1 of window 1 names slot N_SLOTS, one past the pool.
TABLE = [2, 4, 0,
         2, -1, 4,
         2, N_SLOTS, 5]
SENTINEL = 7.0
GROUPS = ("ref_cl", "src_pad", "ref_gmm", "src_gmm", "gin")


class _Guarded:
    """A destination tensor inside a larger buffer filled with SENTINEL, `guard` elements before and after it."""

    def __init__(self, shape, dtype, guard, dev):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * guard,), SENTINEL, dtype=dtype, device=dev)
        self.t = self.buf[guard:guard + n].view(shape)
        self.guard = guard

    def guards_intact(self):
        g = self.guard
        return bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[-g:] == SENTINEL).all())


@pytest.mark.parametrize("feat_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("F", [16, 64])
def test_gather_views_against_torch_indexing(hip_lib, gpu, F, feat_dtype):
    g = torch.Generator().manual_seed(1000 + F)
    dt = torch.bfloat16 if feat_dtype == "bf16" else torch.float32
    # seeded values everywhere, the borders included: src_pad must carry whole padded frames and ref_cl must strip the border
    feat = torch.randn((N_SLOTS, H + 2, W + 2, F), generator=g).to(dt).to(gpu)
    gmm = torch.randn((N_SLOTS, 2, H, W), generator=g).to(gpu)
    xhi = torch.randn((N_SLOTS, R, 256), generator=g).to(torch.bfloat16).to(gpu)
    xlo = torch.randn((N_SLOTS, R, 256), generator=g).to(torch.bfloat16).to(gpu)
    slots = torch.tensor(TABLE, dtype=torch.int32, device=gpu)
    assert (2 * H * W * 4) % 16 != 0                               # (mu, sigma) frames do not keep 16-byte alignment

    def frame(pool, s):
        return pool[s] if 0 <= s < N_SLOTS else torch.zeros_like(pool[0])

    exp = {"ref_cl": torch.stack([frame(feat, s)[1:-1, 1:-1] for s in TABLE[:B]]),
           "src_pad": torch.stack([frame(feat, s) for s in TABLE[B:]]),
           "ref_gmm": torch.stack([frame(gmm, s) for s in TABLE[:B]]),
           "src_gmm": torch.stack([frame(gmm, s) for s in TABLE[B:]]),
           "gin_hi": torch.cat([frame(xhi, s) for s in TABLE[:B]]),
           "gin_lo": torch.cat([frame(xlo, s) for s in TABLE[:B]])}
    assert not exp["src_pad"][1].any() and not exp["src_pad"][V * B - 2].any() and exp["src_gmm"][0].any()

    # Guards of the (mu, sigma) destinations, in floats.  A pool frame is 280 bytes, so slot s sits 0 (s even) or 8 (s odd) bytes past a
    # 16-byte boundary.  Odd guards (3, 5) put every destination frame at 4 or 12: no frame is misaligned like its source, all go
    # float by float.  Guards (2, 4) put ref_gmm's frames at 8, 0, 8 and src_gmm's at 0, 8, 0, 8, 0, 8: frame 1 of ref_gmm (slot 4)
    # is aligned with its source, and frame 5 of src_gmm (slot 5) shares its source's 8 bytes: a head of two floats, a vector body
    # and a tail of two.  The feature and G-Net destinations always start on a boundary.
    for skip, (g_ref, g_src) in [(None, (3, 5)), (None, (2, 4))] + [(grp, (3, 5)) for grp in GROUPS]:
        d = {"ref_cl": _Guarded((B, H, W, F), dt, 64, gpu), "src_pad": _Guarded((V * B, H + 2, W + 2, F), dt, 64, gpu),
             "ref_gmm": _Guarded((B, 2, H, W), torch.float32, g_ref, gpu), "src_gmm": _Guarded((V * B, 2, H, W), torch.float32, g_src, gpu),
             "gin_hi": _Guarded((B * R, GIN_LD), torch.bfloat16, 64, gpu), "gin_lo": _Guarded((B * R, GIN_LD), torch.bfloat16, 64, gpu)}
        if (g_ref, g_src) == (2, 4):
            assert gmm[5].data_ptr() % 16 == d["src_gmm"].t[5].data_ptr() % 16 == 8 and TABLE[B + 5] == 5
            assert gmm[4].data_ptr() % 16 == d["ref_gmm"].t[1].data_ptr() % 16 == 0 and TABLE[1] == 4
        kw = {k: d[k].t for k in GROUPS[:4] if k != skip}
        if skip != "gin":
            kw["gin"] = (d["gin_hi"].t, d["gin_lo"].t, GIN_LD, C_OFF)
        lib.gather_views(slots, B, V, pool_feat=feat, pool_gmm=gmm, pool_xd3=(xhi, xlo), **kw)
        torch.cuda.synchronize()
        for name, dst in d.items():
            assert dst.guards_intact(), (skip, name)
            group = "gin" if name.startswith("gin") else name
            if group == skip:
                assert bool((dst.t == SENTINEL).all()), (skip, name)           # a group left out is not touched
            elif group == "gin":
                assert _same(dst.t[:, C_OFF:C_OFF + 256], exp[name]), (skip, name)
                assert bool((dst.t[:, :C_OFF] == SENTINEL).all()) and bool((dst.t[:, C_OFF + 256:] == SENTINEL).all()), (skip, name)
            else:
                assert _same(dst.t, exp[name]), (skip, name)


def test_gather_views_argument_errors(hip_lib, gpu):
    pool = FramePool(2, H, W, 16, "fp32", gpu)
    slots = torch.zeros(3, dtype=torch.int32, device=gpu)
    gin = torch.zeros((R, GIN_LD), dtype=torch.bfloat16, device=gpu)
    with pytest.raises(lib.MagnetError, match="multiples of 8"):
        lib.gather_views(slots, 1, 2, pool_gmm=pool.gmm, pool_xd3=(pool.xd3_hi, pool.xd3_lo), gin=(gin, gin.clone(), GIN_LD, 60))
    with pytest.raises(lib.MagnetError, match="expected"):
        lib.gather_views(slots, 1, 2, pool_feat=pool.feat, ref_cl=torch.zeros((1, H, W, 8), device=gpu))
    with pytest.raises(lib.MagnetError, match="slots has shape"):
        lib.gather_views(slots, 2, 2, pool_gmm=pool.gmm, ref_gmm=torch.zeros((2, 2, H, W), device=gpu))


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------------
class PerImage(nn.Module):
    """Runs `fn` one image at a time and counts the images: a frame's backbone outputs cannot depend on the batch it came in."""

    def __init__(self, inner, fn=None):
        super().__init__()
        self.inner = inner
        self.fn = fn
        self.count = 0

    def forward(self, img):
        self.count += img.shape[0]
        outs = [(self.fn or self.inner)(img[i:i + 1]) for i in range(img.shape[0])]
        if isinstance(outs[0], (list, tuple)):                      # the encoder's feature list (entries no decoder reads are None)
            return [None if o is None else torch.cat([x[k] for x in outs]) for k, o in enumerate(outs[0])]
        return torch.cat(outs)


T, IMG = 6, 256
# windows with V = 2 neighbours at offsets -1 / +1, B = 2 windows per call, walked over the sequence and then back to its start:
# with the whole sequence in the pool the third call encodes nothing; a pool of 4 frames has dropped frames 0 and 1 by then
CALLS = ([1, 2], [3, 4], [1, 2])


class Frozen(nn.Module):
    """Runs `inner` one image at a time and computes an image's outputs once: later calls repeat them.  The torch decoder's
    convolutions are not reproducible from run to run on the GPU (MAGNET.forward with dnet_backend='torch' differed from itself by
    2.3e-6 on identical inputs), so a bit-for-bit comparison of two paths that both call it needs the frames' outputs pinned."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.memo = {}
        self.count = 0

    def forward(self, img):
        self.count += img.shape[0]
        outs = []
        for i in range(img.shape[0]):
            key = img[i].cpu().numpy().tobytes()
            if key not in self.memo:
                self.memo[key] = self.inner(img[i:i + 1])
            outs.append(self.memo[key])
        return tuple(torch.cat(parts) for parts in zip(*outs))


def _model(gpu, D, dnet_backend="hip", wrap_dnet=None):
    args = make_args(D=D, iters=2, dpv_h=IMG // 4, dpv_w=IMG // 4, fdim=64, V=2)
    args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
    f = fnet.FNET(args)
    seeded_fnet_state(f.f_net, seed=5)
    f = f.to(gpu).eval()
    f_runner = fnet.FNetMFMA(f.f_net)
    d = make_dnet(seed=2, enc_seed=3)
    d.d_net.encoder = PerImage(d.d_net.encoder)
    if wrap_dnet is not None:
        d = wrap_dnet(d)
    model = MAGNET(args, d_net=d, f_net=PerImage(f, f_runner.run), feat_dtype="bf16", dnet_backend=dnet_backend).to(gpu).eval()
    seeded_magnet_weights(model, seed=4, gain=0.3)
    return model


def _counts(model):
    return model.d_net.d_net.encoder.count, model.f_net.count


def _sequence(gpu):
    g = torch.Generator().manual_seed(77)
    frames = torch.rand(T, 3, IMG, IMG, generator=g).to(gpu)
    calls = []
    for refs in CALLS:
        nghbrs = [r - 1 for r in refs] + [r + 1 for r in refs]      # view-major: v B + b
        gp = torch.Generator().manual_seed(500 + refs[0])           # a call's poses depend on its windows alone
        calls.append((refs, nghbrs, synth.make_poses("scannet", len(refs), 2, gp).to(gpu), torch.ones(len(refs), 2, dtype=torch.int32),
                      synth.make_intrinsics("scannet", IMG // 4, IMG // 4, len(refs))))
    return frames, calls


def _run_calls(step, frames, calls):
    with torch.no_grad():
        return [[p.clone() for p in step(refs, frames[refs], nghbrs, frames[nghbrs], poses, valid, intr)] for refs, nghbrs, poses, valid, intr in calls]


def _all_same(got, ref):
    return len(got) == len(ref) and all(len(g) == len(r) and all(_same(x, y) for x, y in zip(g, r)) for g, r in zip(got, ref))


@pytest.mark.parametrize("D", [5, 64])
def test_sequence_runner_equals_magnet_forward(hip_lib, gpu, D):
    model = _model(gpu, D)
    frames, calls = _sequence(gpu)
    nB = len(CALLS[0])

    # non-triviality, on the MAGNET.forward side alone: the cost volume of the first call from the backbones' outputs
    refs, nghbrs, poses, valid, intr = calls[0]
    with torch.no_grad():
        imgs = torch.cat((frames[refs], frames[nghbrs]))
        gmms, _ = model._dnet(model.d_net.d_net.encoder(imgs))
        feats = model.f_net(imgs)
        cost = torch.empty((nB, D, IMG // 4, IMG // 4), device=gpu)
        CostVolumeCW(feats[:nB], feats[nB:], gmms[nB:], poses, valid, intr, 5, feat_dtype="bf16")(ref_gmm=gmms[:nB], k_list=model.k_list, out=cost)
    nonzero = float((cost != 0).float().mean())
    print(f"D = {D}: {nonzero:.3f} of the first call's cost-volume entries are non-zero")
    assert nonzero >= 0.1
    model.d_net.d_net.encoder.count = model.f_net.count = 0

    # the reference: MAGNET.forward on every call, B (1 + V) images each
    ref = _run_calls(lambda ri, rimg, ni, nimg, *rest: model(rimg, nimg, *rest, mode="test"), frames, calls)
    assert _counts(model) == (len(CALLS) * nB * 3,) * 2
    assert all(len(r) == 2 and bool(torch.isfinite(p).all()) for r in ref for p in r)
    assert not _same(ref[0][-1], ref[1][-1])
    model.d_net.d_net.encoder.count = model.f_net.count = 0

    # (a), (b): every prediction of every window, and T images encoded in total
    runner = SequenceRunner(model, capacity=T)
    got = _run_calls(runner.forward, frames, calls)
    assert _all_same(got, ref)
    assert _counts(model) == (T, T) and runner.encoded == T

    # (c) negative control: two neighbour ids of the first call swapped (views 0 and 1 of window 0: frames 0 and 2)
    swapped = list(nghbrs)
    swapped[0], swapped[nB] = swapped[nB], swapped[0]
    with torch.no_grad():
        right = runner.refine(refs, nghbrs, poses, valid, intr)
        assert _all_same([right], ref[:1])
        wrong = runner.refine(refs, swapped, poses, valid, intr)
    assert not _same(wrong[-1], ref[0][-1])
    assert _counts(model) == (T, T)                                 # refine encodes nothing

    # (d) a pool below T: frames 0 and 1 are evicted by the second call and encoded again for the third
    model.d_net.d_net.encoder.count = model.f_net.count = 0
    small = SequenceRunner(model, capacity=4)
    got = _run_calls(small.forward, frames, calls)
    assert _all_same(got, ref)
    assert _counts(model) == (T + 2, T + 2) and small.encoded == T + 2
    with torch.no_grad(), pytest.raises(lib.MagnetError, match="6 distinct frames"):
        small.add(list(range(T)), frames)


# ---- 3. the torch-backbone form: the pack route into the pool --------------------------------------------------------------------
def test_sequence_runner_torch_backbones(hip_lib, gpu):
    model = _model(gpu, 5, dnet_backend="torch", wrap_dnet=Frozen)
    model.fnet_mfma = False
    frames, calls = _sequence(gpu)
    refs, nghbrs, *rest = calls[0]                                  # the first call of the walk: 4 distinct frames in 6 images
    with torch.no_grad():
        # the comparison presupposes that MAGNET.forward repeats itself to the bit (see Frozen)
        ref = [p.clone() for p in model(frames[refs], frames[nghbrs], *rest, mode="test")]
        again = model(frames[refs], frames[nghbrs], *rest, mode="test")
        print("MAGNET.forward against itself, max |difference|:", max(float((x - y).abs().max()) for x, y in zip(again, ref)))
        assert _all_same([again], [ref])
        runner = SequenceRunner(model, capacity=8)
        got = runner.forward(refs, frames[refs], nghbrs, frames[nghbrs], *rest)
    print("SequenceRunner.forward against MAGNET.forward, max |difference|:", max(float((x - y).abs().max()) for x, y in zip(got, ref)))
    assert _all_same([got], [ref]) and runner.encoded == 4 and model.d_net.count == 6 + 6 + 4
    # a pool whose free slots are not consecutive goes through the staging planes: five held frames, the second one used last, so
    # that the four new frames take slots 0, 2, 3, 4
    staged = SequenceRunner(model, capacity=5)
    staged.pool = FramePool(5, IMG // 4, IMG // 4, 64, "bf16", gpu)
    staged.pool.assign(["held%d" % i for i in range(5)])
    staged.pool.slots(["held1"])
    with torch.no_grad():
        got = staged.forward(refs, frames[refs], nghbrs, frames[nghbrs], *rest)
    assert staged.pool.slots([1, 2, 0, 3]) == [0, 2, 3, 4] and "held1" in staged.pool
    assert _all_same([got], [ref])


def test_fnet_runner_route_fills_the_pool(hip_lib, gpu):
    """The matrix-core F-Net's outputs live in its own reused buffers: add() copies them into the slots."""
    args = make_args(D=5, iters=1, dpv_h=IMG // 4, dpv_w=IMG // 4, fdim=64, V=2)
    args.FNET_architecture, args.FNET_feature_dim = "PSM-Net", 64
    f = fnet.FNET(args)
    seeded_fnet_state(f.f_net, seed=5)
    model = MAGNET(args, d_net=StubDNet(1), f_net=f, feat_dtype="bf16").to(gpu).eval()
    frames, _ = _sequence(gpu)
    runner = SequenceRunner(model, capacity=4)
    f_run = model._fnet_runner()
    assert f_run is not None
    exp = {"feat": [], "gmm": [], "hi": [], "lo": []}
    with torch.no_grad():
        # the expected values come from the same batches add() encodes: first occurrences (a, b, c), then d alone
        for ids, imgs, sel in ((["a", "b", "a", "c"], frames[[0, 1, 0, 2]], frames[:3]), (["c", "d"], frames[2:4], frames[3:4])):
            assert runner.add(ids, imgs) == sel.shape[0]
            exp["feat"].append(f_run.run(sel, n_ref=0, feat_dtype="bf16")[1].clone())
            gmm, x_d3 = model.d_net(sel)
            hi, lo = (torch.zeros((sel.shape[0] * 66 * 66, 256), dtype=torch.bfloat16, device=gpu) for _ in range(2))
            lib.pack_split(x_d3.float().contiguous(), hi, lo, 256, 0)
            exp["gmm"].append(gmm); exp["hi"].append(hi); exp["lo"].append(lo)
    pool = runner.pool
    assert pool.slots(["a", "b", "c", "d"]) == [0, 1, 2, 3] and runner.encoded == 4
    assert _same(pool.feat, torch.cat(exp["feat"])) and _same(pool.gmm, torch.cat(exp["gmm"]))
    assert _same(pool.xd3_hi.view(-1, 256), torch.cat(exp["hi"])) and _same(pool.xd3_lo.view(-1, 256), torch.cat(exp["lo"]))
    assert bool(pool.feat.any()) and bool(pool.xd3_lo.any())


def test_failed_add_leaves_no_frame_behind(hip_lib, gpu):
    """A D-Net that fails after the slots were assigned: the new ids are gone again, the old frames are untouched."""
    args = make_args(D=5, iters=1, dpv_h=8, dpv_w=8, fdim=16, V=2)
    model = MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=16)).to(gpu).eval()
    good = model.d_net

    class Narrow(StubDNet):
        def forward(self, img):
            gmm, x = super().forward(img)
            return gmm, x[:, :128]

    imgs = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(gpu)
    runner = SequenceRunner(model, capacity=3)
    with torch.no_grad():
        assert runner.add(["a", "b"], imgs[:2]) == 2
        held = runner.pool.gmm.clone()
        model.d_net = Narrow(1).to(gpu).eval()
        with pytest.raises(lib.MagnetError, match="x_d3"):
            runner.add(["a", "c"], torch.cat((imgs[:1], imgs[2:])))
        assert "c" not in runner.pool and runner.pool.slots(["a", "b"]) == [0, 1] and runner.encoded == 2
        assert _same(runner.pool.gmm, held)
        with pytest.raises(lib.MagnetError, match="'c'"):
            runner.refine(["a"], ["b", "c"], None, None, None)
        model.d_net = good
        assert runner.add(["c"], imgs[2:]) == 1 and runner.pool.slots(["c"]) == [2]


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------
class PerImageStubDNet(StubDNet):
    def forward(self, img):
        outs = [StubDNet.forward(self, img[i:i + 1]) for i in range(img.shape[0])]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


class PerImageStubFNet(StubFNet):
    def forward(self, img):
        return torch.cat([StubFNet.forward(self, img[i:i + 1]) for i in range(img.shape[0])])


def test_eval_driver_reuse_backbones_writes_the_same_metrics(hip_lib, gpu, tmp_path, monkeypatch):
    """eval_synthetic.py over a folder of 6 frames, 4 windows that share frames, with and without --reuse_backbones: the same
    metrics file.  The driver's stand-in backbones are torch convolutions whose results depend on the batch they run in (with the
    stock stand-ins the two files differed in the 7th digit: abs_diff 0x1.28be8ebb1be00p+1 against 0x1.28be875800d60p+1), so, as in
    the end-to-end test, they run one image at a time here; the driver's command line is run in this process for that."""
    import PIL  # noqa: F401  (the scene builder needs it; a missing library is a failure here, not a skip)
    import eval_synthetic
    from magnet_amd import sequence, standin
    runners = []

    class Recorded(SequenceRunner):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            runners.append(self)
    monkeypatch.setattr(sequence, "SequenceRunner", Recorded)
    monkeypatch.setattr(standin, "StubDNet", PerImageStubDNet)
    monkeypatch.setattr(standin, "StubFNet", PerImageStubFNet)
    _make_scene(str(tmp_path), "scene0002_00", 6, raw_wh=(96, 64))
    split = tmp_path / "split.txt"
    split.write_text("".join(f"scene0002_00 {i}\n" for i in (1, 2, 3, 4)))
    outs = []
    for extra in ([], ["--reuse_backbones", "--pool_frames", "6"]):
        path = tmp_path / ("metrics%d.json" % len(outs))
        monkeypatch.setattr(sys, "argv", ["eval_synthetic.py", "--dataset_path", str(tmp_path), "--split", str(split), "--V", "2", "--D", "8",
                                          "--iters", "2", "--batch", "2", "--window_radius", "1", "--input_height", "64",
                                          "--input_width", "96", "--sharded", "--dump_metrics", str(path)] + extra)
        eval_synthetic.main()
        outs.append(path.read_text())
    assert '"frames": 4' in outs[0] and "nan" not in outs[0].lower()
    assert outs[0] == outs[1]
    # frames were reused: the 2 calls of 2 windows name 6 images each and the 6 frames of the folder between them
    assert len(runners) == 1 and runners[0].encoded == 6 and len(runners[0].pool) == 6
