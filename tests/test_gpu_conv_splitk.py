"""-m gpu: the split-K form of the plain bf16x3 layer (magnet_conv_mfma_splitk; csrc/conv_mfma.hip: conv_mfma_splitk_kernel and
conv_splitk_reduce_kernel).

The partials are checked WITHOUT a tolerance: work[z] must equal what the existing launch writes to out_f32 for that channel range
alone (channel-offset input view, weights packed for the range, zero bias, no activation).  The final output is then checked bit for
bit against the fixed-order fp32 sum of those partials + bias + LeakyReLU in every output form the decoder uses, and pointwise against
fp64 with the bound of tests/conv_fwd_ref.py lengthened by the S additions of the reduce:
    |got - ref| <= 1.01 x 2^-16 x M + gamma(3 K + 4 + S) x (M + |bias|),   M = |x| conv |w|, K = taps x cin
(LeakyReLU carried through as conv_fwd_ref carries it).

Shape: 2 images of a 13 x 15 interior = 2 x 15 x 17 = 510 rows: three full 128-row tiles and a ragged one, the image boundary inside a
tile; cout_pad 256 = two N tiles.  cin 160 = 5 chunks (S = 2: 3 + 2) and cin 512 = 16 chunks (S = 3: 5 + 5 + 6; S = 8: 2 each, the
chunk minimum), 3x3 and 1x1."""
import pytest
import torch
import torch.nn.functional as F

from magnet_amd import lib
from magnet_amd.planes import pack_taps, split_bf16
from tests.conv_fwd_ref import LOLO, U, conv_ref, f32, gamma_l, interior, join, ratio

pytestmark = pytest.mark.gpu

N, H, W, COUT = 2, 13, 15, 256
HP, WP = H + 2, W + 2
ROWS = N * HP * WP
SLOPE = 0.01
SENT = 7.0
GUARD = 4096
CASES = [(9, 160, 2), (9, 512, 3), (9, 512, 8), (1, 160, 2), (1, 512, 3), (1, 512, 8)]
_cache = {}


def _ranges(cin, S):
    C = cin // 32
    return [(z * C // S * 32, (z + 1) * C // S * 32) for z in range(S)]


def _setup(gpu, taps, cin, S):
    """Inputs, the reference partials (existing launch per channel range) and the expected pre-activation sum, computed once."""
    key = (taps, cin, S)
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(100 * taps + cin + S)
    k = 3 if taps == 9 else 1
    x = torch.randn(N, H, W, cin, generator=g)
    wt = torch.randn(COUT, cin, k, k, generator=g) / (k * cin ** 0.5)
    bias = (torch.randn(COUT, generator=g) * 0.5).to(gpu)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1)).reshape(ROWS, cin).to(gpu)
    xh, xl = split_bf16(xp)
    wh, wl = pack_taps(wt.to(gpu))
    zero = torch.zeros(COUT, device=gpu)
    parts = []
    for c0, c1 in _ranges(cin, S):
        o = torch.full((ROWS, COUT), SENT, device=gpu)
        lib.conv_mfma(xh[:, c0:], xl[:, c0:], cin, c1 - c0, wh[:, :, c0:c1].contiguous(), wl[:, :, c0:c1].contiguous(), zero, taps, WP,
                      False, ROWS, out_f32=o)
        parts.append(o)
    acc = parts[0].clone()
    for p in parts[1:]:
        acc = acc + p                                                   # fp32, ascending z
    pre = acc + bias
    act = torch.where(pre < 0, pre * torch.tensor(SLOPE, dtype=torch.float32, device=gpu), pre)
    inner = interior(N, HP, WP, 1, gpu)
    exp = torch.where(inner[:, None], act, torch.zeros_like(act))       # border positions: +0
    assert float((act < 0).float().mean()) > 0.3
    _cache[key] = dict(xh=xh, xl=xl, wh=wh, wl=wl, bias=bias, parts=parts, exp=exp, inner=inner)
    return _cache[key]


def _work(gpu, S):
    full = torch.full((S * ROWS * COUT + GUARD,), SENT, device=gpu)
    return full, full[:S * ROWS * COUT]


def _run(d, taps, cin, S, work, **kw):
    return lib.conv_mfma(d["xh"], d["xl"], cin, cin, d["wh"], d["wl"], d["bias"], taps, WP, False, ROWS, leaky=SLOPE, border=(HP, 1),
                         split_k=S, work=work, **kw)


@pytest.mark.parametrize("taps,cin,S", CASES)
def test_partials_are_the_existing_launch_on_each_channel_range(hip_lib, gpu, taps, cin, S):
    d = _setup(gpu, taps, cin, S)
    full, work = _work(gpu, S)
    out = torch.full((ROWS, COUT), SENT, device=gpu)
    tiles = _run(d, taps, cin, S, work, out_f32=out)
    assert tiles == (ROWS + 127) // 128
    got = work.reshape(S, ROWS, COUT)
    for z in range(S):
        assert torch.equal(got[z], d["parts"][z]), f"partial {z} of {S} differs from the launch on its channel range"
    # the ragged tile's rows >= ROWS of the last split would land behind the workspace: nothing there is written
    assert (full[S * ROWS * COUT:] == SENT).all()


@pytest.mark.parametrize("form", ["planes", "f32", "repad", "slice"])
@pytest.mark.parametrize("taps,cin,S", CASES)
def test_final_output_is_the_fixed_order_sum_bitwise(hip_lib, gpu, taps, cin, S, form):
    d = _setup(gpu, taps, cin, S)
    _, work = _work(gpu, S)
    exp = d["exp"]
    if form == "f32":
        buf = torch.full((ROWS + 8, COUT), SENT, device=gpu)            # 8 guard rows behind the output
        _run(d, taps, cin, S, work, out_f32=buf[:ROWS])
        assert torch.equal(buf[:ROWS], exp) and (buf[ROWS:] == SENT).all()
        assert not buf[:ROWS][~d["inner"]].any()                        # border zeros
    elif form == "repad":
        buf = torch.full((N * H * W + 8, COUT), SENT, device=gpu)
        _run(d, taps, cin, S, work, out_f32=buf[:N * H * W].reshape(N, H, W, COUT), repad=1)
        assert torch.equal(buf[:N * H * W], exp[d["inner"]]) and (buf[N * H * W:] == SENT).all()
    else:
        ctot, off = (COUT, 0) if form == "planes" else (384, 64)
        oh = torch.full((ROWS + 8, ctot), SENT, dtype=torch.bfloat16, device=gpu); ol = torch.full_like(oh, SENT)
        _run(d, taps, cin, S, work, out_hi=oh[:ROWS, off:], out_lo=ol[:ROWS, off:], out_ld=ctot if form == "slice" else 0)
        eh, el = split_bf16(exp)
        for got, e in ((oh, eh), (ol, el)):
            assert torch.equal(got[:ROWS, off:off + COUT].view(torch.int16), e.view(torch.int16))
            assert (got[ROWS:] == SENT).all()
            assert (got[:ROWS, :off] == SENT).all() and (got[:ROWS, off + COUT:] == SENT).all()     # nothing outside the slice


@pytest.mark.parametrize("taps,cin,S", CASES)
def test_pointwise_against_fp64(hip_lib, gpu, taps, cin, S):
    d = _setup(gpu, taps, cin, S)
    _, work = _work(gpu, S)
    out = torch.empty((ROWS, COUT), device=gpu)
    _run(d, taps, cin, S, work, out_f32=out)
    K = taps * cin
    ref, b0 = conv_ref(join(d["xh"], d["xl"]), join(d["wh"], d["wl"]), taps, WP, ROWS)
    mag = b0 / (1.01 * LOLO + 1.02 * gamma_l(3 * K + 2))                 # conv_ref's |x| conv |w|
    bias = d["bias"].double()
    ref = ref + bias
    bound = 1.01 * LOLO * mag + gamma_l(3 * K + 4 + S) * (mag + bias.abs())
    s = f32(SLOPE)
    neg = ref - bound < 0
    bound = max(1.0, abs(s)) * bound + torch.where(neg, U * abs(s) * (ref.abs() + bound), torch.zeros_like(bound))
    ref = torch.where(ref < 0, ref * s, ref)
    inner = d["inner"]
    worst, i = ratio(out[inner], ref[inner], bound[inner])
    print(f"split-K taps {taps} cin {cin} S {S}: worst |error| / bound = {worst:.3g}")
    assert worst <= 1.0


def test_refusals_on_the_device_write_nothing(hip_lib, gpu):
    taps, cin, S = 9, 160, 2
    d = _setup(gpu, taps, cin, S)
    full, work = _work(gpu, S)
    out = torch.full((ROWS, COUT), SENT, device=gpu)
    _run(d, taps, cin, S, work, out_f32=out)                            # the valid launch
    assert torch.equal(out, d["exp"])
    full.fill_(SENT); out.fill_(SENT)
    ob = torch.full((ROWS, COUT), SENT, dtype=torch.bfloat16, device=gpu)
    wh4 = d["wh"][:4].contiguous(); wl4 = d["wl"][:4].contiguous()
    zeros = torch.zeros(ROWS, COUT, device=gpu)

    def refused(code, S_=S, work_=work, taps_=taps, wh=d["wh"], wl=d["wl"], **kw):
        kw.setdefault("out_f32", out)
        with pytest.raises(lib.MagnetError) as e:
            lib.conv_mfma(d["xh"], d["xl"], cin, cin, wh, wl, d["bias"], taps_, WP, False, ROWS, leaky=SLOPE, border=(HP, 1),
                          split_k=S_, work=work_, **kw)
        assert e.value.code == code, e.value
    refused(lib.E_DIM, S_=9)
    refused(lib.E_DIM, S_=1)
    refused(lib.E_DIM, S_=3)                                            # 5 chunks over 3 splits: one would get a single chunk
    refused(lib.E_DIM, work_=work[:-4])                                 # too small
    refused(lib.E_ALIGN, work_=full[1:1 + work.numel()])
    refused(lib.E_DIM, tiling=lib.TILING_BM64)
    refused(lib.E_DIM, tiling=lib.TILING_BM256)
    refused(lib.E_DIM, out_f32=None, out_bf16=ob)                       # out_mode 2
    refused(lib.E_DIM, taps_=4, wh=wh4, wl=wl4)
    refused(lib.E_DIM, repad=-1)                                        # the base checks apply
    torch.cuda.synchronize()
    assert (full == SENT).all() and (out == SENT).all() and (ob == SENT).all()
    # the existing entry points refuse what they refused: a split-K workspace means nothing to them
    with pytest.raises(lib.MagnetError):
        lib.conv_mfma(d["xh"], d["xl"], cin, cin, d["wh"], d["wl"], d["bias"], taps, WP, False, ROWS, out_f32=out, addend=zeros,
                      split_k=S, work=work)
    assert (out == SENT).all()


def test_two_runs_are_bit_identical(hip_lib, gpu):
    taps, cin, S = 9, 512, 3
    d = _setup(gpu, taps, cin, S)
    res = []
    for _ in range(2):
        _, work = _work(gpu, S)
        oh = torch.empty((ROWS, COUT), dtype=torch.bfloat16, device=gpu); ol = torch.empty_like(oh)
        _run(d, taps, cin, S, work, out_hi=oh, out_lo=ol)
        res.append((work.clone(), oh, ol))
    assert all(torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
               for a, b in zip(*res))
