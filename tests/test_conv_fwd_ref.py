"""CPU: the fp64 restatements of tests/conv_fwd_ref.py equal torch float64 convolutions on bordered grids; an fp32 emulation of the
kernel's arithmetic (bf16 planes, three partial products per 32-wide K chunk, fp32 accumulation in the kernel's order) stays inside
the derived bounds; and each of seven planted defects of that emulation exceeds the bound somewhere.  (That the 2x2 window is the
space-to-depth form of a stride-2 3x3 is shown by tests/test_fnet_bwd_ref.py::test_s2d_refs_are_stride2_autograd on the same
tap_offsets / conv_ref; here the window is checked against a plain 2x2 correlation.)"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from magnet_amd.convnet import split_bf16
from magnet_amd.planes import pack_taps
from tests import conv_fwd_ref as C


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _grid(x_nchw, pad):
    """(N, C, h, w) -> the zero-bordered channel-last rows (N*(h+2pad)*(w+2pad), C)."""
    N, Cc, h, w = x_nchw.shape
    out = torch.zeros((N, h + 2 * pad, w + 2 * pad, Cc), dtype=x_nchw.dtype)
    out[:, pad:pad + h, pad:pad + w] = x_nchw.permute(0, 2, 3, 1)
    return out.reshape(-1, Cc)


def _interior(rows, N, h, w, pad):
    return rows.reshape(N, h + 2 * pad, w + 2 * pad, -1)[:, pad:pad + h, pad:pad + w].permute(0, 3, 1, 2)


def _taps64(wt):
    """(cout, cin, k, k) fp64 -> (k*k, cout, cin)."""
    return wt.permute(2, 3, 0, 1).reshape(-1, wt.shape[0], wt.shape[1]).contiguous()


# ---- the restatements against float64 torch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 2), (1, 1)])
@pytest.mark.parametrize("epi", ["none", "residual", "addend", "relu", "leaky-neg", "leaky-big"])
def test_conv_fwd_ref_is_conv2d(k, dil, epi):
    N, cin, cout, h, w, pad = 2, 8, 16, 7, 9, 2
    x = torch.randn(N, cin, h, w, generator=_g(1), dtype=torch.float64)
    wt = torch.randn(cout, cin, k, k, generator=_g(2), dtype=torch.float64)
    b = torch.randn(cout, generator=_g(3), dtype=torch.float64)
    r = torch.randn(N, cout, h, w, generator=_g(4), dtype=torch.float64)
    rows, wp = N * (h + 2 * pad) * (w + 2 * pad), w + 2 * pad
    slope = {"leaky-neg": -0.375, "leaky-big": 2.5}.get(epi)        # fp32-exact slopes
    ref, bound = C.conv_fwd_ref(_grid(x, pad), _taps64(wt), b, k * k, wp, rows, dil=dil,
                                addend=_grid(r, pad) if epi == "addend" else None, add=_grid(r, pad) if epi == "residual" else None,
                                relu=epi == "relu", leaky=slope)
    exp = F.conv2d(x, wt, b, padding=dil * (k // 2), dilation=dil)
    if epi in ("addend", "residual"):
        exp = exp + r
    if epi == "relu":
        exp = F.relu(exp)
    if slope is not None:
        exp = F.leaky_relu(exp, slope)
    torch.testing.assert_close(_interior(ref, N, h, w, pad), exp, rtol=1e-12, atol=1e-12)
    assert (bound > 0).all() and bound.shape == ref.shape


def test_conv_fwd_ref_2x2_window_is_a_2x2_correlation():
    """taps = 4 reads (-1,-1), (-1,0), (0,-1), (0,0): the 2x2 correlation whose window ENDS at the position."""
    N, cin, cout, h, w, pad = 2, 8, 16, 6, 7, 1
    x = torch.randn(N, cin, h, w, generator=_g(5), dtype=torch.float64)
    wt = torch.randn(cout, cin, 2, 2, generator=_g(6), dtype=torch.float64)
    b = torch.randn(cout, generator=_g(7), dtype=torch.float64)
    ref, _ = C.conv_fwd_ref(_grid(x, pad), _taps64(wt), b, 4, w + 2, N * (h + 2) * (w + 2))
    exp = F.conv2d(F.pad(x, (1, 0, 1, 0)), wt, b)
    torch.testing.assert_close(_interior(ref, N, h, w, pad), exp, rtol=1e-12, atol=1e-12)


def test_addend_and_residual_exclude_each_other():
    z = torch.zeros(4, 8, dtype=torch.float64)
    with pytest.raises(ValueError):
        C.conv_fwd_ref(z, torch.zeros(1, 8, 8, dtype=torch.float64), torch.zeros(8), 1, 3, 4, addend=z, add=z)


@pytest.mark.parametrize("repad", [0, 1, 2])
def test_border_and_repad_addressing(repad):
    N, cin, cout, h, w, pad = 3, 8, 8, 5, 6, 2
    x = torch.randn(N, cin, h, w, generator=_g(8), dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=_g(9), dtype=torch.float64)
    b = torch.randn(cout, generator=_g(10), dtype=torch.float64)
    hp, wp = h + 2 * pad, w + 2 * pad
    ref, bound = C.conv_fwd_ref(_grid(x, pad), _taps64(wt), b, 9, wp, N * hp * wp)
    assert ref.reshape(N, hp, wp, cout)[:, 0].abs().min() > 0           # the bias reaches the border rows of the plain form
    img, bimg, written = C.border_and_repad(ref, bound, N, hp, wp, pad, repad)
    conv = F.conv2d(x, wt, b, padding=1)
    q = pad if repad == 0 else repad - 1
    exp = F.pad(conv, (q, q, q, q)).permute(0, 2, 3, 1).reshape(-1, cout)
    assert img.shape == exp.shape == bimg.shape
    torch.testing.assert_close(img, exp, rtol=1e-12, atol=1e-12)
    inner = C.interior(N, h + 2 * q, w + 2 * q, q)
    assert torch.equal(written, inner if repad else torch.ones_like(inner))
    assert (bimg[~inner] == 0).all() and (img[~inner] == 0).all() and (bimg[inner] > 0).all()


def _tail_params(tail_cout, seed, positive=False):
    """The three 1x1 layers.  positive: heavy-tailed non-negative weights and positive biases — no cancellation in W a, so |W| e is
    what an input error really does and the interval bound is sharp (with signed weights the sums cancel and the bound, which cannot
    know that, is orders of magnitude above any fp32 error: sound, but blind to a low-order defect)."""
    g = _g(seed)
    if positive:
        ws = [(torch.randn(n, 128, 1, 1, generator=g) ** 3).abs() / 128 for n in (128, 128, tail_cout)]
        bs = [torch.randn(n, generator=g).abs() * 0.5 + 0.01 for n in (128, 128, tail_cout)]
    else:
        ws = [torch.randn(n, 128, 1, 1, generator=g) / 128 ** 0.5 for n in (128, 128, tail_cout)]
        bs = [torch.randn(n, generator=g) * 0.5 for n in (128, 128, tail_cout)]
    return ws, bs


@pytest.mark.parametrize("tail_cout", [16, 144])
def test_tail_ref_is_a_sequential_of_1x1_layers(tail_cout):
    ws, bs = _tail_params(tail_cout, 11)
    seq = nn.Sequential(nn.Conv2d(128, 128, 1), nn.ReLU(), nn.Conv2d(128, 128, 1), nn.ReLU(), nn.Conv2d(128, tail_cout, 1)).double()
    with torch.no_grad():
        for m, wv, bv in zip((seq[0], seq[2], seq[4]), ws, bs):
            m.weight.copy_(wv.double()); m.bias.copy_(bv.double())
        a0 = torch.randn(37, 128, generator=_g(12), dtype=torch.float64)
        exp = seq(a0.t().reshape(1, 128, 37, 1)).reshape(tail_cout, 37).t()
    ref, bound = C.tail_ref(a0, torch.zeros_like(a0), torch.cat([wv.double().reshape(-1) for wv in ws]), torch.cat(bs), tail_cout)
    torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)
    _, wider = C.tail_ref(a0, torch.full_like(a0, 1e-3), torch.cat([wv.double().reshape(-1) for wv in ws]), torch.cat(bs), tail_cout)
    assert (bound > 0).all() and (wider > bound).all()                 # an input error widens every output's bound


# ---- the fp32 emulation of the kernel's arithmetic ------------------------------------------------------------------------------
def _shift(x, off, rows):
    """x[off:off + rows] with rows outside [0, len(x)) read as zero."""
    out = torch.zeros((rows, x.shape[1]), dtype=x.dtype)
    a, b = max(off, 0), min(off + rows, x.shape[0])
    if b > a:
        out[a - off:b - off] = x[a:b]
    return out


def emulate_conv(xh, xl, wh, wl, bias, taps, wp, rows, dil=1, addend=None, add=None, relu=False, leaky=None, defect=None):
    """conv_mfma's plain launch in fp32: K chunk outer, tap inner, per (chunk, tap) lo hi, hi lo, hi hi into one fp32 accumulator, then
    ((acc + ad) + bias) and the activation.  defect: one of the planted faults (None: the kernel as written)."""
    xh, xl, wh, wl = xh.float(), xl.float(), wh.float(), wl.float()
    cout, cin = wh.shape[1], wh.shape[2]
    offs = C.tap_offsets(taps, wp, dil)
    acc = torch.zeros((rows, cout), dtype=torch.float32)
    for k0 in range(0, cin, 32):
        for t, off in enumerate(offs):
            if defect == "tap_one_column_off" and t == 5 % taps:
                off += 1
            ah, al = _shift(xh[:, k0:k0 + 32], off, rows), _shift(xl[:, k0:k0 + 32], off, rows)
            bh, bl = wh[t][:, k0:k0 + 32], wl[t][:, k0:k0 + 32]
            if not (defect == "lo_hi_dropped" and t == 4 % taps and k0 == 32 * ((cin // 32) // 2)):
                acc = acc + al @ bh.T
            acc = acc + ah @ bl.T
            acc = acc + ah @ bh.T
    ad = torch.zeros_like(acc)
    if add is not None:
        ad = add[0].float()[:rows, :cout] + (0 if defect == "residual_lo_ignored" else add[1].float()[:rows, :cout])
    if addend is not None:
        ad = addend.float()[:rows, :cout]
    b = bias.float().clone()
    if defect == "bias_group_missing":
        b[8:16] = 0
    v = (acc + ad) + b
    if relu:
        v = v.clamp_min(0.0)
    elif leaky is not None:
        s = torch.tensor(C.f32(leaky), dtype=torch.float32)
        v = v * s if defect == "leaky_on_positive" else torch.where(v < 0, v * s, v)
    if defect == "last_tile_from_the_tile_before":
        r0 = (rows - 1) // 128 * 128
        v = v.clone()
        v[r0:] = v[r0 - 128:rows - 128]
    return v


def emulate_tail(a0, tail_wh, tail_wl, tail_bias, tail_cout, defect=None):
    """The fused tail in fp32 from the fp32 activation a0 (rows, 128) (split here, as the first layer's epilogue does;
    planes split again are unchanged): per layer and 32-wide chunk hi_w lo_a, lo_w hi_a, hi_w hi_a, then bias, ReLU, re-split."""
    hi, lo = split_bf16(a0.float())
    wo = bo = 0
    for layer, n in enumerate((128, 128, tail_cout)):
        Wh = tail_wh.float().reshape(-1)[wo:wo + n * 128].reshape(n, 128)
        Wl = tail_wl.float().reshape(-1)[wo:wo + n * 128].reshape(n, 128)
        b = tail_bias.float()[bo:bo + n]
        wo, bo = wo + n * 128, bo + n
        ah, al = hi.float(), lo.float()
        acc = torch.zeros((a0.shape[0], n), dtype=torch.float32)
        for k0 in range(0, 128, 32):
            acc = acc + al[:, k0:k0 + 32] @ Wh[:, k0:k0 + 32].T
            acc = acc + ah[:, k0:k0 + 32] @ Wl[:, k0:k0 + 32].T
            acc = acc + ah[:, k0:k0 + 32] @ Wh[:, k0:k0 + 32].T
        v = acc + b
        if layer == 2:
            return v
        hi, lo = split_bf16(v.clamp_min(0.0))
        if defect == "hidden_activation_hi_only" and layer == 1:
            lo = torch.zeros_like(lo)


def _heavy(shape, seed, scale=1.0):
    """Heavy-tailed values (a sign-keeping cube of a normal): single terms dominate some outputs, as after a ReLU with outliers."""
    return torch.randn(shape, generator=_g(seed)) ** 3 * scale


def _plain_case(taps, cin, cout, dil=1, seed=0, N=2, h=9, w=13, heavy=True):
    """Planes of a zero-bordered grid (border = dil), the pack, a non-zero bias, a residual and an addend; 330 or 442 rows."""
    pad = max(dil, 1)
    hp, wp = h + 2 * pad, w + 2 * pad
    rows = N * hp * wp
    make = _heavy if heavy else (lambda s, sd, scale=1.0: torch.randn(s, generator=_g(sd)) * scale)
    xg = torch.zeros((N, hp, wp, cin))
    xg[:, pad:pad + h, pad:pad + w] = make((N, h, w, cin), 100 + seed)
    k = {9: 3, 4: 2, 1: 1}[taps]
    wt = make((cout, cin, k, k), 200 + seed, (taps * cin) ** -0.5)
    xh, xl = split_bf16(xg.reshape(rows, cin))
    wh, wl = pack_taps(wt)
    bias = torch.randn(cout, generator=_g(300 + seed)) * 0.5
    res = split_bf16(make((rows, cout), 400 + seed))
    addend = make((rows, cout), 500 + seed)
    return dict(xh=xh, xl=xl, wh=wh, wl=wl, bias=bias, taps=taps, wp=wp, rows=rows, dil=dil, res=res, addend=addend,
                inner=C.interior(N, hp, wp, pad), grid=(N, hp, wp, pad))


def _ref_of(c, **kw):
    add = kw.pop("add", None)
    return C.conv_fwd_ref(C.join(c["xh"], c["xl"]), C.join(c["wh"], c["wl"]), c["bias"], c["taps"], c["wp"], c["rows"], dil=c["dil"],
                          add=None if add is None else C.join(*add), **kw)


def _emu_of(c, **kw):
    return emulate_conv(c["xh"], c["xl"], c["wh"], c["wl"], c["bias"], c["taps"], c["wp"], c["rows"], dil=c["dil"], **kw)


PLAIN = [(9, 64, 128, 1), (9, 32, 16, 2), (4, 128, 64, 1), (1, 320, 144, 1), (9, 320, 32, 1)]


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("taps,cin,cout,dil", PLAIN)
def test_fp32_emulation_of_the_plain_forms_stays_inside_the_bound(taps, cin, cout, dil, heavy):
    c = _plain_case(taps, cin, cout, dil, seed=taps + cin, heavy=heavy)
    worst = {}
    for name, kw in (("plain", {}), ("relu", dict(relu=True)), ("residual", dict(add=c["res"])), ("addend", dict(addend=c["addend"])),
                     ("leaky -0.3", dict(leaky=-0.3)), ("leaky 1.7", dict(leaky=1.7, add=c["res"]))):
        ref, bound = _ref_of(c, **kw)
        worst[name] = C.check(name, _emu_of(c, **kw), ref, bound)
    print(f"[emulation taps={taps} cin={cin} cout={cout} dil={dil} heavy={heavy}] worst ratio " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert min(worst.values()) > 0                                     # the emulation is not the fp64 reference in disguise


def _tail_case(tail_cout, seed, heavy=True, taps=9, cin=64):
    c = _plain_case(taps, cin, 128, 1, seed=seed, heavy=heavy)
    ws, bs = _tail_params(tail_cout, 600 + seed, positive=heavy)
    planes = [pack_taps(wv) for wv in ws]
    c["twh"] = torch.cat([p[0].reshape(-1) for p in planes]); c["twl"] = torch.cat([p[1].reshape(-1) for p in planes])
    c["tb"] = torch.cat(bs); c["tail_cout"] = tail_cout
    return c


def _tail_ref_of(c, addend=None):
    a0, b0 = _ref_of(c, relu=True, addend=addend)
    return C.tail_ref(a0, C.split_bound(a0, b0), C.join(c["twh"], c["twl"]), c["tb"], c["tail_cout"])


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("tail_cout", [16, 128, 144])
def test_fp32_emulation_of_the_tail_stays_inside_the_bound(tail_cout, heavy):
    c = _tail_case(tail_cout, seed=tail_cout, heavy=heavy)
    worst = {}
    for name, addend in (("tail", None), ("tail + addend", c["addend"])):
        ref, bound = _tail_ref_of(c, addend)
        got = emulate_tail(_emu_of(c, relu=True, addend=addend), c["twh"], c["twl"], c["tb"], tail_cout)
        worst[name] = C.check(name, got, ref, bound)
    # the tail on an input that IS planes: bound0 = 0
    a_hi, a_lo = split_bf16(_emu_of(c, relu=True))
    ref, bound = C.tail_ref(C.join(a_hi, a_lo), torch.zeros(a_hi.shape, dtype=torch.float64), C.join(c["twh"], c["twl"]), c["tb"], tail_cout)
    worst["planes"] = C.check("planes", emulate_tail(a_hi.float() + a_lo.float(), c["twh"], c["twl"], c["tb"], tail_cout), ref, bound)
    print(f"[emulation tail_cout={tail_cout} heavy={heavy}] worst ratio " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert min(worst.values()) > 0


# ---- planted defects: each must exceed the bound somewhere -------------------------------------------------------------------------
DEFECTS = [("lo_hi_dropped", {}), ("tap_one_column_off", {}), ("residual_lo_ignored", dict(add=True)), ("bias_group_missing", {}),
           ("leaky_on_positive", dict(leaky=0.9375)), ("last_tile_from_the_tile_before", {})]


@pytest.mark.parametrize("taps,cin,cout,dil", [(9, 64, 128, 1), (9, 32, 144, 2), (4, 128, 64, 1), (1, 32, 16, 1)])
@pytest.mark.parametrize("defect,kw", DEFECTS, ids=[d for d, _ in DEFECTS])
def test_checker_rejects_a_planted_defect_of_the_plain_form(defect, kw, taps, cin, cout, dil):
    """Inputs: heavy-tailed activations and weights (single terms dominate some outputs, where a wrong low-order term is a large
    share of the bound) on the default 330-row grid; the LeakyReLU slope 0.9375 is the subtle case (6 % off on positive values).
    Interior positions only, as the GPU tests compare them."""
    c = _plain_case(taps, cin, cout, dil, seed=7)
    kw = dict(kw)
    if kw.pop("add", False):
        kw["add"] = c["res"]
    ref, bound = _ref_of(c, **kw)
    inner = c["inner"]
    assert C.check("sound", _emu_of(c, **kw)[inner], ref[inner], bound[inner]) <= 1.0
    bad = _emu_of(c, defect=defect, **kw)
    w, _ = C.ratio(bad[inner], ref[inner], bound[inner])
    n_bad = int((((bad.double() - ref).abs() > bound) & inner[:, None]).sum())
    print(f"[defect {defect} taps={taps} cin={cin} cout={cout}] worst ratio {w:.3g}, {n_bad} positions over the bound")
    assert w > 1.0
    with pytest.raises(AssertionError):
        C.check(defect, bad[inner], ref[inner], bound[inner])


@pytest.mark.parametrize("taps,cin", [(9, 64), (1, 32)])
@pytest.mark.parametrize("tail_cout", [16, 128, 144])
def test_checker_rejects_a_hidden_tail_activation_kept_as_hi_only(tail_cout, taps, cin):
    """Non-negative tail weights (see _tail_params): with signed ones this defect reaches 2 % of the bound and is not seen."""
    c = _tail_case(tail_cout, seed=7, taps=taps, cin=cin)
    ref, bound = _tail_ref_of(c)
    a0 = _emu_of(c, relu=True)
    assert C.check("sound", emulate_tail(a0, c["twh"], c["twl"], c["tb"], tail_cout), ref, bound) <= 1.0
    bad = emulate_tail(a0, c["twh"], c["twl"], c["tb"], tail_cout, defect="hidden_activation_hi_only")
    w, _ = C.ratio(bad, ref, bound)
    print(f"[defect hidden_activation_hi_only tail_cout={tail_cout} taps={taps} cin={cin}] worst ratio {w:.3g}")
    assert w > 1.0
