"""The D-Net's EfficientNet-B5 encoder on the HIP path (magnet_amd/encoder.py, csrc/enc_kernels.hip, MAGNET_ACT_SILU): every launch on
its own, pointwise against the fp64 restatements and derived bounds of tests/encoder_ref.py; then the whole encoder and the whole
D-Net against the torch modules at the project's backbone bar (2e-4 of the largest magnitude).  Each test prints its
largest error as a fraction of the bound."""
import functools

import pytest
import torch

from tests import encoder_ref as R
from tests.conv_fwd_ref import check_planes_exact

pytestmark = pytest.mark.gpu
BAR = 2e-4


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def _planes_gpu(x_nchw, c_pad, gpu):
    hi, lo = R.split_planes(R.to_grid(x_nchw, c_pad))
    return hi.to(gpu), lo.to(gpu), R.join(hi, lo)


def _nan_planes(rows, c, gpu):
    (bh, hi), (bl, lo) = (R.guarded((rows, c), gpu, torch.bfloat16) for _ in range(2))
    return bh, hi, bl, lo


def _guards_untouched(name, *bufs):
    for b in bufs:
        assert bool(torch.isnan(b[:R.GUARD].float()).all()) and bool(torch.isnan(b[-R.GUARD:].float()).all()), f"{name}: wrote outside its buffer"


def _border_untouched(name, plane, N, h, w):
    g = torch.isnan(plane.float()).reshape(N, h + 2, w + 2, -1).cpu()
    assert bool(g[:, 0].all() and g[:, -1].all() and g[:, :, 0].all() and g[:, :, -1].all()), f"{name}: a border row was written"
    assert not bool(g[:, 1:-1, 1:-1].any()), f"{name}: an interior element was not written"


# ---- depthwise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(9, 13), (18, 26), (37, 70)])
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("C,c_pad", [(48, 64), (144, 160)])
def test_dwconv_against_fp64(hip_lib, gpu, C, c_pad, k, stride, h, w):
    from magnet_amd import lib
    N = 2
    x = _rand((N, C, h, w), 11 * h + k + stride, 1.5)
    hi, lo, xj = _planes_gpu(x, c_pad, gpu)
    wgt = torch.zeros((k * k, c_pad)); wgt[:, :C] = _rand((k * k, C), 5 + k, 0.4)
    bias = torch.zeros(c_pad); bias[:C] = _rand((C,), 6 + k, 0.3)
    (pt, _), (pl, _) = R.same_pad(h, k, stride), R.same_pad(w, k, stride)
    ho, wo = -(-h // stride), -(-w // stride)
    bh, ohi, bl, olo = _nan_planes(N * (ho + 2) * (wo + 2), c_pad, gpu)
    n_part = lib.dwconv_parts(ho, wo)
    assert n_part == -(-ho // R.TILE_H) * -(-wo // R.TILE_W)
    bp, part = R.guarded((N, n_part, c_pad), gpu)
    assert lib.dwconv_cl(hi, lo, c_pad, N, h, w, c_pad, wgt.to(gpu), bias.to(gpu), k, stride, pt, pl, ohi, olo, c_pad, part) == n_part
    torch.cuda.synchronize()
    name = f"dwconv k{k} s{stride} {h}x{w} C{C}"
    _guards_untouched(name, bh, bl, bp)
    _border_untouched(name, ohi, N, ho, wo)
    _border_untouched(name, olo, N, ho, wo)
    ref, b32, bpl = R.dwconv_ref(R.interior(xj, N, h, w), wgt, bias, k, stride, pt, pl)
    got = R.interior(R.join(ohi.cpu(), olo.cpu()), N, ho, wo)
    worst = R.check(name, got, ref, bpl)
    assert bool((got[:, C:] == 0).all()), f"{name}: pad lanes not zero"
    pref, pb = R.dw_partials_ref(ref, b32)
    wp = R.check(name + " partials", part.cpu().double(), pref, pb)
    mean_ref = ref.sum((2, 3)) / (ho * wo)
    wm = R.check(name + " means", part.cpu().double().sum(1) / (ho * wo), mean_ref, pb.sum(1) / (ho * wo))
    print(f"{name}: outputs {worst:.3f}, partials {wp:.3f}, means {wm:.3f} of the bound")


# ---- gate and scale ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Rr", [(48, 12), (1056, 44), (3072, 128)])
def test_se_gate_and_scale_against_fp64(hip_lib, gpu, C, Rr):
    from magnet_amd import lib
    N, h, w = 2, 5, 7
    c_pad = (C + 31) // 32 * 32
    x = _rand((N, C, h, w), C, 1.0)
    x[1] = x[1] * 0.5 + 0.8                                       # two different images: a wrong image index shows
    hi, lo, xj = _planes_gpu(x, c_pad, gpu)
    n_part = 3
    part = torch.zeros((N, n_part, c_pad)); part[:, :, :C] = _rand((N, n_part, C), C + 1, 6.0)
    part[1] += 2.0
    w1, b1 = _rand((Rr, C), C + 2, (2.0 / C) ** 0.5), _rand((Rr,), C + 3, 0.1)
    w2t, b2 = _rand((Rr, C), C + 4, (2.0 / Rr) ** 0.5), _rand((C,), C + 5, 0.1)
    dev = [t.to(gpu) for t in (part, w1, b1, w2t, b2)]
    gates = []
    for _ in range(2):
        bg, gate = R.guarded((N, c_pad), gpu)
        lib.se_gate(dev[0], n_part, h * w, dev[1], dev[2], dev[3], dev[4], C, Rr, gate)
        torch.cuda.synchronize()
        _guards_untouched("se_gate", bg)
        gates.append(gate.clone())
    assert torch.equal(gates[0], gates[1]), "se_gate: two calls differ"
    gref, gb = R.se_gate_ref(part, h * w, w1, b1, w2t, b2, C, c_pad)
    wg = R.check(f"se_gate C{C} R{Rr}", gates[0].cpu().double(), gref, gb)
    assert bool((gates[0][:, C:] == 0).all()), "se_gate: pad lanes not zero"
    assert float((gates[0][0, :C] - gates[0][1, :C]).abs().max()) > 1e-3       # the two images' gates differ
    # scale, out of place and in place
    rows = N * (h + 2) * (w + 2)
    bh, ohi, bl, olo = _nan_planes(rows, c_pad, gpu)
    lib.se_scale(hi, lo, c_pad, gates[0], N, h, w, c_pad, ohi, olo, c_pad)
    ihi, ilo = hi.clone(), lo.clone()
    lib.se_scale(ihi, ilo, c_pad, gates[0], N, h, w, c_pad, ihi, ilo, c_pad)
    torch.cuda.synchronize()
    _guards_untouched("se_scale", bh, bl)
    _border_untouched("se_scale", ohi, N, h, w)
    sref, sb = R.se_scale_ref(R.interior(xj, N, h, w), gates[0].cpu())
    ws = R.check(f"se_scale C{C}", R.interior(R.join(ohi.cpu(), olo.cpu()), N, h, w), sref, sb)
    inner = R.join(ihi.cpu(), ilo.cpu()).reshape(N, h + 2, w + 2, -1)
    assert torch.equal(R.interior(R.join(ihi.cpu(), ilo.cpu()), N, h, w), R.interior(R.join(ohi.cpu(), olo.cpu()), N, h, w)), "in place differs"
    assert bool((inner[:, 0] == 0).all() and (inner[:, -1] == 0).all() and (inner[:, :, 0] == 0).all() and (inner[:, :, -1] == 0).all())
    print(f"se C{C} R{Rr}: gate {wg:.3f}, scale {ws:.3f} of the bound")


# ---- stem --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 72, 104), (1, 3, 71, 103)])
def test_stem_against_fp64(hip_lib, gpu, shape):
    from magnet_amd import lib
    N, _, H, W = shape
    img = torch.rand(shape, generator=torch.Generator().manual_seed(H))
    wgt, bias = _rand((48, 27), 1, 0.3), _rand((48,), 2, 0.2)
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    bh, ohi, bl, olo = _nan_planes(N * (H2 + 2) * (W2 + 2), 64, gpu)
    lib.enc_stem(img.to(gpu), wgt.to(gpu), bias.to(gpu), ohi, olo)
    torch.cuda.synchronize()
    _guards_untouched("stem", bh, bl)
    _border_untouched("stem", ohi, N, H2, W2)
    got = R.interior(R.join(ohi.cpu(), olo.cpu()), N, H2, W2)
    ref, b = R.stem_ref(img, wgt, bias)
    worst = R.check(f"stem {H}x{W}", got[:, :48], ref, b)
    assert bool((got[:, 48:] == 0).all()), "stem: channels 48..63 not zero"
    print(f"stem {H}x{W}: {worst:.3f} of the bound")


# ---- MAGNET_ACT_SILU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(64, 32), (160, 64), (512, 2048)])
def test_conv_silu_against_fp64(hip_lib, gpu, cin, cout):
    from magnet_amd import lib
    from magnet_amd.planes import split_bf16
    N, h, w = 2, 9, 13
    hp, wp = h + 2, w + 2
    rows = N * hp * wp
    x = _rand((N, cin, h, w), cin, 1.0)
    xhi, xlo, xj = _planes_gpu(x, cin, gpu)
    wf = _rand((1, cout, cin), cout, (2.0 / cin) ** 0.5)
    whi, wlo = split_bf16(wf)
    wj = R.join(whi, wlo)
    bias = _rand((cout,), cout + 1, 0.2)
    res = _rand((N, cout, h, w), cout + 2, 1.0)
    rhi, rlo, rj = _planes_gpu(res, cout, gpu)
    inner = torch.zeros((N, hp, wp), dtype=torch.bool); inner[:, 1:-1, 1:-1] = True
    inner = inner.reshape(-1, 1)
    dev = dict(w_hi=whi.to(gpu), w_lo=wlo.to(gpu), bias=bias.to(gpu))
    worst = 0.0
    for with_res in (False, True):
        add = (rhi, rlo, cout) if with_res else None
        # out_mode 0 (planes) with border_hp: border rows exactly zero
        bh, ohi, bl, olo = _nan_planes(rows, cout, gpu)
        lib.conv_mfma(xhi, xlo, cin, cin, dev["w_hi"], dev["w_lo"], dev["bias"], 1, wp, False, rows, out_hi=ohi, out_lo=olo, add=add,
                      border=(hp, 1), silu=True)
        # out_mode 1 (fp32), no border form: every row is the plain epilogue
        bf, of32 = R.guarded((rows, cout), gpu)
        lib.conv_mfma(xhi, xlo, cin, cin, dev["w_hi"], dev["w_lo"], dev["bias"], 1, wp, False, rows, out_f32=of32, add=add, silu=True)
        # act = 0 on the same arguments through the _ex entry point: today's bits (the plain entry point's)
        b0, o0 = R.guarded((rows, cout), gpu)
        b1, o1 = R.guarded((rows, cout), gpu)
        lib.conv_mfma(xhi, xlo, cin, cin, dev["w_hi"], dev["w_lo"], dev["bias"], 1, wp, False, rows, out_f32=o0, add=add)
        lib.conv_mfma(xhi, xlo, cin, cin, dev["w_hi"], dev["w_lo"], dev["bias"], 1, wp, False, rows, out_f32=o1, add=add, tiling=lib.TILING_FLAT)
        torch.cuda.synchronize()
        _guards_untouched("conv silu", bh, bl, bf, b0, b1)
        assert torch.equal(o0, o1), "act = 0 through magnet_conv_mfma_ex differs from magnet_conv_mfma"
        ref, b = R.conv_silu_ref(xj, wj, bias, rows, add=rj if with_res else None, planes=False)
        worst = max(worst, R.check(f"silu fp32 {cin}->{cout} res={with_res}", of32.cpu().double(), ref, b))
        # the pre-activation is what act = 0 writes: SiLU of it, to the stated accuracy (independent of the K loop's error)
        pre = o0.cpu().double()
        s = pre * torch.sigmoid(pre)
        R.check(f"silu of the launch's own pre-activation {cin}->{cout}", of32.cpu().double(), s, R.SILU_REL * s.abs() + R.SILU_ABS)
        refp, bp = R.conv_silu_ref(xj, wj, bias, rows, add=rj if with_res else None, planes=True)
        z = torch.zeros_like(refp)
        worst = max(worst, R.check(f"silu planes {cin}->{cout} res={with_res}", R.join(ohi.cpu(), olo.cpu()),
                                   torch.where(inner, refp, z), torch.where(inner, bp, z)))
    print(f"conv silu {cin}->{cout}: {worst:.3f} of the bound")


# ---- the whole encoder, the whole D-Net ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoder_case(H, W):
    """The seeded encoder, two different images, and the same module's fp64 and fp32 CPU forwards (computed once, never changed)."""
    from magnet_amd.encoder import Encoder, load_seeded_encoder
    enc = load_seeded_encoder(Encoder(backend="hip"), 0).eval()
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = torch.rand((2, 3, H, W), generator=g)
    img[1] = img[1] * 0.6 + 0.3 * torch.rand((3, 1, 1), generator=g)
    ref = Encoder()
    ref.load_state_dict(enc.state_dict())
    ref.eval()
    with torch.no_grad():
        f32 = ref(img)
        f64 = ref.double()(img.double())
    return enc, img, f64, f32


@pytest.mark.parametrize("H,W", [(72, 104), (64, 96)])
def test_encoder_matches_fp64_forward(hip_lib, gpu, H, W):
    from magnet_amd.encoder import TAPS
    enc, img, f64, f32 = _encoder_case(H, W)
    enc = enc.to(gpu)
    with torch.no_grad():
        got = enc(img.to(gpu))
        one = [enc(img[i:i + 1].to(gpu)) for i in range(2)]
    assert len(got) == 16 and got[0].shape == img.shape and all(got[i] is None for i in range(16) if i not in (0,) + TAPS)
    fails = []
    for i in TAPS:
        top = float(f64[i].abs().max())
        e_hip = float((got[i].cpu().double() - f64[i]).abs().max()) / top
        e_t32 = float((f32[i].double() - f64[i]).abs().max()) / top
        print(f"encoder {H}x{W} tap [{i}] {tuple(got[i].shape)}: max |x| {top:.3g}; HIP {e_hip:.3g}, torch fp32 {e_t32:.3g} of it (bar {BAR:g})")
        assert got[i].shape == f64[i].shape and bool(torch.isfinite(got[i]).all())
        if not e_hip <= BAR:
            fails.append((i, e_hip, e_t32))
        for n in range(2):
            assert torch.equal(one[n][i][0], got[i][n]), f"tap [{i}]: image {n} alone differs from image {n} in the batch"
    assert not fails, f"taps over the bar (index, HIP, torch fp32): {fails}"


def test_whole_dnet_on_hip_matches_torch(hip_lib, gpu):
    from magnet_amd.dnet import DNET, load_seeded_decoder
    from magnet_amd.encoder import Encoder
    from magnet_amd.standin import make_dnet_args
    enc, img, _, _ = _encoder_case(64, 96)
    hip = DNET(make_dnet_args(), Encoder(backend="hip"), dnet=True, backend="hip")
    hip.d_net.encoder.load_state_dict(enc.state_dict())
    load_seeded_decoder(hip.d_net.decoder, 0)
    ref = DNET(make_dnet_args(), Encoder(), dnet=True)
    ref.load_state_dict(hip.state_dict())
    hip, ref = hip.to(gpu).eval(), ref.to(gpu).eval()
    with torch.no_grad():
        a, b = hip(img.to(gpu)), ref(img.to(gpu))
    assert a.shape == b.shape == (2, 2, 64, 96) and bool(torch.isfinite(a).all())
    for c, name in ((0, "mu"), (1, "variance")):
        top = float(b[:, c].abs().max())
        err = float((a[:, c] - b[:, c]).abs().max()) / top
        print(f"whole D-Net {name}: max {top:.3g}, HIP - torch {err:.3g} of it (bar {BAR:g})")
        assert err <= BAR, (name, err)
