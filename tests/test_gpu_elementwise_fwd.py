"""-m gpu: every element-wise forward launch of the default inference step, one direct lib.* launch per case, against the fp64
restatements of tests/elementwise_fwd_ref.py, pointwise (|got - ref| <= bound at every element through `check`; the bounds are derived
there, not measured).  Outputs live inside one allocation with NaN guard bands on both sides (the idiom of tests/test_gpu_conv_fwd.py):
every element of the output region must have been written, nothing outside it may change.  Inputs, cases and seeds come from the
reference module and are the ones tests/test_elementwise_fwd_ref.py runs its fp32 emulations and planted defects on.

These launches are also the anchor of the fused Gaussian update and the fused upsampling inside conv_mfma, which existing tests tie bit
for bit to "the plain tail + the stand-alone kernel" (see the docstring of tests/test_gpu_conv_fwd.py).

E_NATIVE = 1 ulp: the error of the hardware exp2 behind __expf in upsample_kernel / upsample_cl_kernel, the one figure of the bounds
that is measured and not derived: 0.782712 ulp worst over every fp32 input in [-128, 0] (tools/native_exp2_probe.hip on an MI355X,
2026-10-20; the vendor's installed documentation does not state it), rounded up to the next whole ulp.

Worst |got - ref| / bound per kernel family, measured on an MI355X (the tests print one line per case; above 1 is a failure, and a
ratio far below 1 is what it is: nothing here is tuned towards it):

    family (kernel)                                                   worst ratio
    gaussian_update, _cl (gaussian_update_kernel, _cl_kernel)         0.957   (mu1: two roundings, both near half an ulp)
    upsample_depth, all eight <K, C> (upsample_kernel)                0.526   (<8,2> at 2x6x67; 0.05 .. 0.29 at 1x1x1)
    upsample_depth_cl, _cl_n (upsample_cl_kernel)                     0.396
    dnet_gauss_head                                                   0.440
    fnet_stem / _f16                                                  0.425 / 0.976
    avgpool_cl / _f16                                                 0.270 / 0.935   (k = 16, default format: 0.03 .. 0.06, far below 1)
    upsample_bilinear_cl / _f16                                       0.476 / 0.979
    space_to_depth / _f16, pack_gmm                                   bit for bit
  The `_f16` figures sit just below 1 because their bound is almost entirely the one fp16 rounding of the store (half an ulp, which
  some element always nearly reaches); the default format's store term (2^-16 relative) is sixteen times looser than its half-ulp.
  The whole file takes about 2 s of GPU time.
"""
import numpy as np
import pytest
import torch

from magnet_amd import lib
from magnet_amd.planes import split_bf16, to_f16_sat
from tests import elementwise_fwd_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096                                      # sentinel elements in front of and behind every output buffer
NAN_BITS = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
PLANE_DTYPE = {"planes": torch.bfloat16, "f16": torch.float16}
FMTS = ["planes", "f16"]


def _guarded(shape, gpu, dtype=torch.float32):
    """A NaN-filled tensor with GUARD NaN elements on either side of it (same allocation)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=gpu)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _is_sentinel(t):
    """Elementwise: still the NaN the buffer was filled with, bit for bit."""
    return t.contiguous().view(INT_OF[t.dtype]) == NAN_BITS[t.dtype]


def _assert_written_only(name, buf, body, region=None):
    """The guards keep the sentinel; inside `body` exactly the elements of the boolean mask `region` (default: all) were written."""
    torch.cuda.synchronize()
    assert bool(_is_sentinel(buf[:GUARD]).all() and _is_sentinel(buf[-GUARD:]).all()), f"{name}: write outside the output buffer"
    s = _is_sentinel(body).cpu()
    if region is None:
        assert not bool(s.any()), f"{name}: {int(s.sum())} element(s) of the output were not written"
    else:
        assert not bool(s[region].any()), f"{name}: {int(s[region].sum())} element(s) of the output region were not written"
        assert bool(s[~region].all()), f"{name}: an element outside the output region was written"


def _dev(a, gpu):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).contiguous().to(gpu)


def _code(fn, *args, **kw):
    with pytest.raises(lib.MagnetError) as ei:
        fn(*args, **kw)
    return ei.value.code


_REFS = {}


def _cached(key, fn):
    """A reference computed once, shared by the tests that need it, never modified."""
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def _report(name, worst):
    print(f"[{name}] worst |got - ref| / bound = {worst:.4f}")


# ---- convex upsampling ------------------------------------------------------------------------------------------------------------------
def _up_ref(B, h, w, K, C, P=1):
    def make():
        depth, logits = R.upsample_inputs(B, h, w, K, C, P)
        return (depth, logits) + R.convex_upsample_ref(depth, R.logits_nchw(logits, K))
    return _cached(("up", B, h, w, K, C, P), make)


@pytest.mark.parametrize("B,h,w", R.UPSAMPLE_SHAPES)
@pytest.mark.parametrize("K,C", R.UPSAMPLE_KC)
def test_upsample_depth(hip_lib, gpu, K, C, B, h, w):
    depth, logits, ref, bound = _up_ref(B, h, w, K, C)
    buf, out = _guarded((B, C, K * h, K * w), gpu)
    lib.upsample_depth(_dev(depth[0], gpu), _dev(logits, gpu), K, out=out)
    name = f"upsample_depth<{K},{C}> {B}x{h}x{w}"
    _assert_written_only(name, buf, out)
    _report(name, R.check(name, out.cpu(), ref[0], bound[0]))


def test_upsample_depth_rejects(hip_lib, gpu):
    B, h, w = 1, 2, 3
    d = torch.zeros((B, 2, h, w), device=gpu)
    buf = torch.zeros(B * 2 * 16 * h * w + 8, device=gpu)
    off = buf[1:1 + B * 2 * 16 * h * w].view(B, 2, 4 * h, 4 * w)                       # 4 bytes past a 16-byte boundary
    assert _code(lib.upsample_depth, d, torch.zeros((B, 144, h, w), device=gpu), 4, out=off) == lib.E_ALIGN
    assert _code(lib.upsample_depth, torch.zeros((B, 3, h, w), device=gpu), torch.zeros((B, 144, h, w), device=gpu), 4) == lib.E_DIM
    assert _code(lib.upsample_depth, d, torch.zeros((B, 81, h, w), device=gpu), 3) == lib.E_DIM


def _cl_n(depths, mask_pad, ld, outs, n_pred, B, h, w):
    """magnet_upsample_depth_cl_n itself (lib.upsample_depth_cl_n routes one prediction to the _cl entry point)."""
    lib._launch("magnet_upsample_depth_cl_n", depths, depths.data_ptr(), mask_pad.data_ptr(), int(ld), outs.data_ptr(), int(n_pred), B, h, w)


@pytest.mark.parametrize("B,h,w,ld,n_pred", R.UPSAMPLE_CL_CASES)
def test_upsample_depth_cl_n(hip_lib, gpu, B, h, w, ld, n_pred):
    depth, mask_pad, logits = R.upsample_cl_inputs(B, h, w, ld, n_pred)

    def make():
        return R.convex_upsample_ref(depth, R.logits_cl(mask_pad, ld, B, h, w))
    ref, bound = _cached(("upcl", B, h, w, ld, n_pred), make)
    d, m = _dev(depth, gpu), _dev(mask_pad, gpu)
    buf, out = _guarded((n_pred, B, 2, 4 * h, 4 * w), gpu)
    _cl_n(d, m, ld, out, n_pred, B, h, w)
    name = f"upsample_depth_cl_n {B}x{h}x{w} ld {ld} n_pred {n_pred}"
    _assert_written_only(name, buf, out)
    got = out.cpu()
    _report(name, R.check(name, got, ref, bound))
    # _cl is _cl_n with one prediction, bit for bit
    buf1, out1 = _guarded((B, 2, 4 * h, 4 * w), gpu)
    lib.upsample_depth_cl(d[0], m, ld, out=out1)
    _assert_written_only(name + " (_cl)", buf1, out1)
    bufn, outn = _guarded((1, B, 2, 4 * h, 4 * w), gpu)
    _cl_n(d[:1], m, ld, outn, 1, B, h, w)
    _assert_written_only(name + " (_cl_n, 1)", bufn, outn)
    assert torch.equal(out1.view(torch.int32), outn[0].view(torch.int32)) and torch.equal(out1.view(torch.int32), out[0].view(torch.int32))
    # the NCHW <4, 2> instance on the same values: within the sum of both bounds (the same bound twice: one restatement serves both)
    buf2, out2 = _guarded((B, 2, 4 * h, 4 * w), gpu)
    lib.upsample_depth(d[0], _dev(logits, gpu), 4, out=out2)
    _assert_written_only(name + " (NCHW)", buf2, out2)
    R.check(name + " vs NCHW <4,2>", out2.cpu(), got[0].double(), 2.0 * bound[0])


def test_upsample_depth_cl_rejects(hip_lib, gpu):
    B, h, w = 1, 2, 3
    d = torch.zeros((65, B, 2, h, w), device=gpu)
    m = torch.zeros((B * (h + 2) * (w + 2), 148), device=gpu)
    out = torch.zeros((65, B, 2, 4 * h, 4 * w), device=gpu)
    assert _code(_cl_n, d, m, 148, out, 65, B, h, w) == lib.E_DIM
    assert _code(_cl_n, d, m, 146, out, 2, B, h, w) == lib.E_DIM
    assert _code(lib.upsample_depth_cl, d[0], m, 146) == lib.E_DIM


# ---- Gaussian update, dnet_gauss_head ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,h,w", R.GAUSS_SHAPES)
def test_gaussian_update_both_layouts(hip_lib, gpu, B, h, w):
    o, g = R.gaussian_inputs(B, h, w)
    ref, bound = _cached(("gauss", B, h, w), lambda: R.gaussian_update_ref(o, g))
    gd = _dev(g, gpu)
    buf, out = _guarded((B, 2, h, w), gpu)
    lib.gaussian_update(_dev(o, gpu), gd, out=out)
    name = f"gaussian_update {B}x{h}x{w}"
    _assert_written_only(name, buf, out)
    worst = R.check(name, out.cpu(), ref, bound)
    assert bool((out[:, 1] > 0).all())                                                  # a standard deviation: sg0 > 0 here
    for ld in R.GAUSS_LDS:
        o_pad = _dev(R.pad_cl(o, ld, fill=np.float32("nan")), gpu)                      # border rows and spare channels: poisoned
        bufc, outc = _guarded((B, 2, h, w), gpu)
        lib.gaussian_update_cl(o_pad, ld, gd, h, w, out=outc)
        _assert_written_only(f"{name} cl ld {ld}", bufc, outc)
        assert torch.equal(outc.view(torch.int32), out.view(torch.int32)), f"{name}: the layouts differ at ld {ld}"
    _report(name, worst)


@pytest.mark.parametrize("N,h,w,pad,in_ld", R.GAUSS_HEAD_CASES)
def test_dnet_gauss_head(hip_lib, gpu, N, h, w, pad, in_ld):
    x = R.gauss_head_inputs(N, h, w)
    ref, bound = _cached(("head", N, h, w), lambda: R.gauss_head_ref(x))
    rows = _dev(R.pad_cl(x, in_ld, pad=pad, fill=np.float32("nan")), gpu)                # border rows and spare channels: poisoned
    buf, out = _guarded((N, 2, h, w), gpu)
    lib.dnet_gauss_head(rows, in_ld, N, h, w, pad, out)
    name = f"dnet_gauss_head {N}x{h}x{w} pad {pad} ld {in_ld}"
    _assert_written_only(name, buf, out)
    got = out.cpu()
    assert torch.equal(got[:, 0].view(torch.int32), torch.from_numpy(x[:, 0].copy()).view(torch.int32))       # channel 0: a copy
    _report(name, R.check(name, got, ref, bound))


def test_dnet_gauss_head_rejects(hip_lib, gpu):
    N, h, w = 1, 2, 3
    out = torch.zeros((N, 2, h, w), device=gpu)
    odd = torch.zeros((N * (h + 2) * (w + 2), 5), device=gpu)
    assert _code(lib.dnet_gauss_head, odd, 5, N, h, w, 1, out) == lib.E_DIM
    flat = torch.zeros(N * (h + 2) * (w + 2) * 4 + 4, device=gpu)
    off = flat[1:1 + N * (h + 2) * (w + 2) * 4].view(-1, 4)                              # 4 bytes past an 8-byte boundary
    assert _code(lib.dnet_gauss_head, off, 4, N, h, w, 1, out) == lib.E_ALIGN


# ---- the F-Net's small layers, default two-plane format and the single-plane fp16 format ---------------------------------------------------
def _out_planes(shape, gpu, fmt):
    """Guarded output plane(s) of a format: [(buf, body)] (one for f16, hi and lo for planes)."""
    return [_guarded(shape, gpu, PLANE_DTYPE[fmt]) for _ in range(1 if fmt == "f16" else 2)]


def _value(planes):
    """What the plane(s) hold, in float64 on the host."""
    return sum(body.cpu().double() for _, body in planes)


def _in_planes(x32, gpu, fmt):
    """fp32 values -> the device plane(s) of a format and the float64 values they hold."""
    if fmt == "f16":
        p = to_f16_sat(x32)
        return [p.to(gpu)], p.double()
    hi, lo = split_bf16(x32)
    return [hi.to(gpu), lo.to(gpu)], hi.double() + lo.double()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,H,W", R.STEM_SHAPES)
def test_fnet_stem(hip_lib, gpu, N, H, W, fmt):
    img, wgt, b = R.stem_inputs(N, H, W)
    ref, bound = _cached(("stem", N, H, W, fmt), lambda: R.stem_ref(img, wgt, b, fmt))
    H2, W2 = ref.shape[1:3]
    outs = _out_planes((N, H2 + 2, W2 + 2, 32), gpu, fmt)
    args = (img.to(gpu), wgt.contiguous().to(gpu), b.to(gpu))
    if fmt == "f16":
        lib.fnet_stem_f16(*args, outs[0][1].view(-1, 32))
    else:
        lib.fnet_stem(*args, outs[0][1].view(-1, 32), outs[1][1].view(-1, 32))
    name = f"fnet_stem {fmt} {N}x{H}x{W}"
    region = torch.zeros((N, H2 + 2, W2 + 2, 32), dtype=torch.bool); region[:, 1:-1, 1:-1] = True
    for buf, body in outs:
        _assert_written_only(name, buf, body, region)
    _report(name, R.check(name, _value(outs)[:, 1:-1, 1:-1], ref, bound))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("H2,W2,opad", R.S2D_CASES)
def test_space_to_depth(hip_lib, gpu, H2, W2, opad, fmt):
    N, C = 2, 32
    a, b = R.s2d_inputs(H2, W2, N, C)
    srcs = [to_f16_sat(a)] if fmt == "f16" else [a.to(torch.bfloat16), b.to(torch.bfloat16)]      # hi and lo are moved independently
    ins = []
    for s in srcs:
        p = torch.full((N, H2 + 2, W2 + 2, C), float("nan"), dtype=s.dtype)              # the input grid's border is never read
        p[:, 1:-1, 1:-1] = s
        ins.append(p.reshape(-1, C).to(gpu))
    H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
    outs = _out_planes((N, H4 + 2 * opad, W4 + 2 * opad, 4 * C), gpu, fmt)
    if fmt == "f16":
        lib.space_to_depth_f16(ins[0], outs[0][1].view(-1, 4 * C), N, C, H2, W2, opad)
    else:
        lib.space_to_depth(ins[0], ins[1], outs[0][1].view(-1, 4 * C), outs[1][1].view(-1, 4 * C), N, C, H2, W2, opad)
    name = f"space_to_depth {fmt} {H2}x{W2} opad {opad}"
    region = torch.zeros((N, H4 + 2 * opad, W4 + 2 * opad, 4 * C), dtype=torch.bool); region[:, opad:opad + H4, opad:opad + W4] = True
    for (buf, body), s in zip(outs, srcs):
        _assert_written_only(name, buf, body, region)
        exp = R.space_to_depth_ref(s)
        assert torch.equal(body.cpu()[:, opad:opad + H4, opad:opad + W4].contiguous().view(torch.int16), exp.contiguous().view(torch.int16)), name


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C,k", R.AVGPOOL_CASES)
def test_avgpool_cl(hip_lib, gpu, C, k, fmt):
    N, h, w, pad, ld, c0 = R.AVGPOOL_GRID
    planes, held = _cached(("pool_in", fmt, str(gpu)), lambda: _in_planes(R.avgpool_inputs().reshape(-1, ld), gpu, fmt))
    held = held.reshape(N, h + 2 * pad, w + 2 * pad, ld)
    ref, bound = _cached(("pool", C, k, fmt), lambda: R.avgpool_ref(held[:, pad:-pad, pad:-pad, c0:c0 + C], k, fmt))
    cells = N * (h // k) * (w // k)
    outs = _out_planes((cells, C), gpu, fmt)
    if fmt == "f16":
        lib.avgpool_cl_f16(planes[0][:, c0:c0 + C], ld, N, h, w, pad, k, C, outs[0][1])
    else:
        lib.avgpool_cl(planes[0][:, c0:c0 + C], planes[1][:, c0:c0 + C], ld, N, h, w, pad, k, C, outs[0][1], outs[1][1])
    name = f"avgpool_cl {fmt} C {C} k {k}"
    for buf, body in outs:
        _assert_written_only(name, buf, body)
    _report(name, R.check(name, _value(outs), ref, bound))


@pytest.mark.parametrize("fmt", FMTS)
def test_avgpool_cl_rejects(hip_lib, gpu, fmt):
    dt = PLANE_DTYPE[fmt]
    x = torch.zeros((2 * 23 * 39, 320), dtype=dt, device=gpu)
    out = torch.zeros((64, 136), dtype=dt, device=gpu)

    def run(h, k, C):
        if fmt == "f16":
            lib.avgpool_cl_f16(x, 320, 2, h, 35, 2, k, C, out)
        else:
            lib.avgpool_cl(x, x, 320, 2, h, 35, 2, k, C, out, out)
    assert _code(run, 19, 8, 136) == lib.E_DIM
    assert _code(run, 7, 8, 128) == lib.E_DIM


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ph,pw,h,w,pad", R.BILINEAR_CASES)
def test_upsample_bilinear_cl(hip_lib, gpu, ph, pw, h, w, pad, fmt):
    N, C, ld, c0 = R.BILINEAR_N, R.BILINEAR_C, R.BILINEAR_LD, R.BILINEAR_OFF
    rows = R.bilinear_inputs(ph, pw)                                                     # NaN rows behind the last image: never read
    ref, bound = _cached(("bil", ph, pw, h, w, fmt), lambda: R.bilinear_ref(rows[:N * ph * pw].reshape(N, ph, pw, C), h, w, fmt))
    outs = _out_planes((N, h + 2 * pad, w + 2 * pad, ld), gpu, fmt)
    sl = [body.view(-1, ld)[:, c0:c0 + C] for _, body in outs]
    if fmt == "f16":
        lib.upsample_bilinear_cl_f16(rows.to(gpu), C, ph, pw, C, sl[0], ld, N, h, w, pad)
    else:
        lib.upsample_bilinear_cl(rows.to(gpu), C, ph, pw, C, sl[0], sl[1], ld, N, h, w, pad)
    name = f"upsample_bilinear_cl {fmt} {ph}x{pw} -> {h}x{w} pad {pad}"
    region = torch.zeros((N, h + 2 * pad, w + 2 * pad, ld), dtype=torch.bool); region[:, pad:pad + h, pad:pad + w, c0:c0 + C] = True
    for buf, body in outs:
        _assert_written_only(name, buf, body, region)
    _report(name, R.check(name, _value(outs)[:, pad:pad + h, pad:pad + w, c0:c0 + C], ref, bound))


# ---- pack_gmm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,h,w", R.PACK_GMM_SHAPES)
def test_pack_gmm(hip_lib, gpu, N, h, w):
    g = R.pack_gmm_inputs(N, h, w)
    buf, out = _guarded((N, h + 2, w + 2, 2), gpu)
    lib.pack_gmm(g.to(gpu), out=out)
    _assert_written_only(f"pack_gmm {N}x{h}x{w}", buf, out)
    assert torch.equal(out.cpu().view(torch.int32), R.pack_gmm_ref(g).view(torch.int32))                      # the border: +0, bit for bit
