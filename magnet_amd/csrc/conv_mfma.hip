// conv_mfma.hip — G-Net / mask-head convolutions as implicit GEMM on the bf16 matrix cores with
// bf16x3 operand splitting (row N1 of SURVEY.md §8f; reference: models/MAGNET.py:47-70,111-118).
//
// The reference runs these layers in fp32.  gfx950 has no reduced-precision fp32 matrix path (no xf32)
// and fp32 MFMA runs at the vector rate (157 TF), 1/16 of the bf16 matrix rate.  So every fp32 operand
// is split x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (16 mantissa bits kept) and
//      x*w  ~=  hi_x*hi_w + hi_x*lo_w + lo_x*hi_w          (dropped terms < 2^-16 |x w|)
// is accumulated in fp32 by three v_mfma_f32_16x16x32_bf16 per tile: fp32-grade results (measured
// relative error ~1e-5 on these layers, tests/test_gpu_conv.py) at up to 1/3 of the bf16 matrix peak.
//
// GEMM view:  out[p, n] = bias[n] + sum_{tap, c} act[p + off(tap), c] * W[tap][n][c]
//   p   = row index in the ZERO-BORDERED channel-last activation (B, h+2, w+2, C) flattened over
//         (B, h+2, w+2): with the border in place a 3x3 tap is a plain row offset off = dy*(w+2)+dx and
//         the kernel needs no boundary logic at all.  Border rows are computed too (3 % extra work at
//         120x160) and hold garbage that no interior output ever reads; callers read interior rows only.
//   act = two bf16 planes (hi, lo), W = two bf16 planes of [tap][Cout_pad][Cin] (Cin contiguous), so both
//         MFMA operands are "row-major with K contiguous": one 16-byte LDS read per fragment per lane.
// Tiling: workgroup = 128 rows x BN = NF*16 output channels, 2x2 waves of 64x64 (BN = 128) or 4 waves stacked
// along M (BN = 144, 16), K step 32; global -> registers -> LDS staging with the next step's loads in flight during the
// MFMAs into the other half of a double-buffered, XOR-swizzled (conflict-free) LDS image: one barrier per K
// step; epilogue through LDS: bias, ReLU, then either re-split to bf16 hi/lo planes (input of the next layer)
// or fp32 rows (last layer).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/magnet_hip.h"
#include "conv_common.hpp"
#include "warp_math.hpp"

namespace magnet {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;

[[maybe_unused]] constexpr int CV_BK = 32;
constexpr int CV_ROW = 64;                            // bytes per staged row (32 bf16), unpadded

// LDS image of a [rows][32 bf16] tile: 64-byte rows, the four 16-byte slots of a row XOR-swizzled with
// ((row >> 1) & 3).  Conflict-free for both access patterns (checked against the ds_read_b128 /
// ds_write_b128 lane groups of MI355X_MICROARCH.md §LDS): MFMA fragment reads (lane -> row = lane&15,
// slot = lane>>4) and the staging writes (thread -> row = t>>2, slot = t&3).  The first version used
// 80-byte padded rows: SQ_LDS_BANK_CONFLICT was 50 % of SQ_LDS_IDX_ACTIVE.
__device__ __forceinline__ int cv_swz(int row, int slot) { return row * CV_ROW + ((slot ^ ((row >> 1) & 3)) << 4); }

__device__ __forceinline__ uint16_t bf16_rne(float f) { return f32_to_bf16_rne(f); }     // v_cvt_pk_bf16_f32 (warp_math.hpp)
__device__ __forceinline__ void split_bf16(float x, uint16_t& hi, uint16_t& lo) {
    hi = bf16_rne(x);
    lo = bf16_rne(x - __uint_as_float((uint32_t)hi << 16));
}

// NF = 16-column fragments of the workgroup tile (BN = NF*16: 128, 144 or 16 channels);
// WN = waves along N (2: 2x2 waves; 1: 4x1 waves); CV_BM = rows of the workgroup tile (64, 128 or 256)
// SPB = K stages per barrier interval (the LDS ring holds 2*SPB stages)
__device__ __forceinline__ int act_swz(int row, int slot) { return row * 256 + ((slot ^ (row & 15)) << 4); }

// Arguments of the fused convex upsampling (ConvParams::up_*), passed by value to the last tail layer
struct UpArgs { const float* depth; float* out; int npred, h, w, B; };   // Gaussian update: depth = (mu, sigma) in, out = (mu, sigma) out, npred = -1

// One 1x1 layer of the fused tail over K = 128: activations read from the LDS tile (act_swz layout), weight fragments straight from
// global memory (64 KB per layer, L2-resident; no LDS staging).  Operands are swapped (weights = MFMA A operand): the accumulator is
// C^T — a lane holds 4 CONSECUTIVE output channels of one row.
// Column-owned: wave w computes output fragments n = w, w + 4 (32 of the 128 output channels)
// for ALL rows of the tile, so it fetches a quarter of the layer's weights (16 KB instead of 64 KB per wave: with row ownership the
// two resident workgroups pull 128 KB per K chunk through the CU's 64 B/clk vector-memory path for 1 536 cycles of MFMA work — the
// tails ran at half the K loop's efficiency) and reads every row's activations from LDS (256 B/clk, cheap).  A remainder
// fragment (TAILN % 4 == 1: the 16-channel G-Net head, the 9th fragment of the 144-channel mask head) is row-split over the
// waves.  The layer's output replaces its input in place: one barrier after the last read, one after the last write.
// (Round 4 measured a 2 (row halves) x 4 (column groups) ownership for the 8-wave form — half the fragment reads from LDS, twice the
// weights through the vector-memory path, bit-identical results: 2.07 - 2.09 / 1.90 - 1.93 ms against 2.07 - 2.08 / 1.88 - 1.89 ms for
// this form on the two stacks, same box (profiles/r4/conv_tail_ownership_ab.log).  Not kept: the tails, like the K loop, do not speed
// up by moving load between pipes.)
template <int TAILN, bool LAST, int ROWS, int NW = 4, bool UP = false, bool OPAQUE_LANE = false>
__device__ __forceinline__ void tail_layer_cols(const uint16_t* __restrict__ w_hi, const uint16_t* __restrict__ w_lo,
                                                const float* __restrict__ bias, unsigned char* act_hi, unsigned char* act_lo,
                                                float* __restrict__ out, int out_ld, long long row0, long long rows, int lane, int wv,
                                                const UpArgs up = UpArgs{nullptr, nullptr, 0, 0, 0, 0}) {
    // NW waves: wave w owns output fragments w, w + NW, ...; MA row blocks, read from LDS MB = 8 at a time (all 4 of a 64-row tile)
    constexpr int NJ = TAILN / NW, REM = TAILN % NW, MA = ROWS / 16, MR = MA / NW;   // MR: remainder-fragment row blocks per wave
    // OPAQUE_LANE (the fp16 instances' upsampling layer): this call derives its fragment addresses itself instead of sharing them with
    // the plain last layer in the other branch — kept alive across this one's 256-register peak, two of them went to scratch
    if constexpr (OPAQUE_LANE) asm volatile("" : "+v"(lane));
    constexpr int MB = MA < 8 ? MA : 8;
    static_assert(REM <= 1 && MA % MB == 0 && MA % NW == 0, "one row-split remainder fragment at most");
    f32x4_t acc[NJ > 0 ? NJ : 1][MA], accr[MR];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int m = 0; m < MA; ++m) acc[j][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < MR; ++m) accr[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, kslot = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        if constexpr (NJ > 0) {
            bf16x8_t wh[NJ], wl[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const size_t e = (size_t)((wv + NW * j) * 16 + frow) * 128 + kk * 32 + kslot * 8;
                wh[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(w_hi + e));
                wl[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(w_lo + e));
            }
#pragma unroll
            for (int mb = 0; mb < MA; mb += MB) {
                bf16x8_t xh[MB], xl[MB];
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    xh[m] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(act_hi + act_swz((mb + m) * 16 + frow, kk * 4 + kslot)));
                    xl[m] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(act_lo + act_swz((mb + m) * 16 + frow, kk * 4 + kslot)));
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
#pragma unroll
                    for (int m = 0; m < MB; ++m) acc[j][mb + m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], xl[m], acc[j][mb + m], 0, 0, 0);
#pragma unroll
                    for (int m = 0; m < MB; ++m) acc[j][mb + m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], xh[m], acc[j][mb + m], 0, 0, 0);
#pragma unroll
                    for (int m = 0; m < MB; ++m) acc[j][mb + m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], xh[m], acc[j][mb + m], 0, 0, 0);
                }
            }
        }
        if constexpr (REM) {
            const size_t e = (size_t)(NJ * NW * 16 + frow) * 128 + kk * 32 + kslot * 8;
            const bf16x8_t wh = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(w_hi + e));
            const bf16x8_t wl = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(w_lo + e));
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                const int row = (wv * MR + m) * 16 + frow;
                const bf16x8_t rh = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(act_hi + act_swz(row, kk * 4 + kslot)));
                const bf16x8_t rl = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(act_lo + act_swz(row, kk * 4 + kslot)));
                accr[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, rl, accr[m], 0, 0, 0);
                accr[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, rh, accr[m], 0, 0, 0);
                accr[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, rh, accr[m], 0, 0, 0);
            }
        }
    }
    if constexpr (UP) {
        // ---- learned convex upsampling (models/MAGNET.py:15-27) behind the mask head's last layer, column-owned: the 144 logits of a
        // position sit in 9 different waves (fragment n = neighbour n of the 3x3 window), so they meet in LDS: HR = 128 rows (a 64-row tile: all 64)
        // x 144 fp32 at a time in the (now dead) activation tile and K ring, then one thread per (position, sub-pixel row i) does what upsample_cl_kernel does
        // — same arithmetic, same order: bit-identical — with the mask read from LDS instead of HBM.
        static_assert(TAILN == 9 && LAST && (ROWS % 128 == 0 || ROWS == 64), "mask head's last layer");
        constexpr int HR = ROWS < 128 ? ROWS : 128, HB = HR / 16;   // rows / 16-row blocks of one pass
        constexpr int SP = 148;                               // stage row pitch in floats: 16 rows x 4 quads of a fragment store hit distinct banks
        float* stage = reinterpret_cast<float*>(act_hi);      // HR x 148 x 4 B = 74 KB (37 KB at 64 rows) <= the launch's LDS (launch_conv_nf)
        const int wp = up.w + 2, img_rows = (up.h + 2) * wp;
        const size_t hw = (size_t)up.h * up.w;
        const int tid = wv * 64 + lane;
        for (int half = 0; half < ROWS / HR; ++half) {
            __syncthreads();                                  // every wave is done with the activation tile / with the previous half's stage
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int m = 0; m < MA; ++m) {
                    if (m / HB != half) continue;
                    const int ch = (wv + NW * j) * 16 + (lane >> 4) * 4, srow = (m % HB) * 16 + (lane & 15);
                    const float4 b4 = *reinterpret_cast<const float4*>(bias + ch);
                    *reinterpret_cast<float4*>(stage + srow * SP + ch) =
                        make_float4(acc[j][m][0] + b4.x, acc[j][m][1] + b4.y, acc[j][m][2] + b4.z, acc[j][m][3] + b4.w);
                }
            if constexpr (REM) {
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    const int mrow = wv * MR + m;
                    if (mrow / HB != half) continue;
                    const int ch = NJ * NW * 16 + (lane >> 4) * 4, srow = (mrow % HB) * 16 + (lane & 15);
                    const float4 b4 = *reinterpret_cast<const float4*>(bias + ch);
                    *reinterpret_cast<float4*>(stage + srow * SP + ch) =
                        make_float4(accr[m][0] + b4.x, accr[m][1] + b4.y, accr[m][2] + b4.z, accr[m][3] + b4.w);
                }
            }
            __syncthreads();
            for (int t = tid; t < HR * 4; t += NW * 64) {     // (position of this half, sub-pixel row i): 2 per thread, 1 at 64 rows
                const int srow = t >> 2, i = t & 3;
                const long long row = row0 + half * HR + srow;
                const int b = (int)((unsigned)row / (unsigned)img_rows);                  // rows < 2^31 (checked by the API)
                const int rem = (int)((unsigned)row - (unsigned)b * (unsigned)img_rows);
                const int yy = rem / wp, xx = rem - yy * wp;
                if (row >= rows || yy < 1 || yy > up.h || xx < 1 || xx > up.w) continue;  // border position: nothing to write
                const int y = yy - 1, x = xx - 1;
                const float* mrow = stage + srow * SP + i * 4;
                float4 mv[9];
                float4 mx = make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
#pragma unroll
                for (int n = 0; n < 9; ++n) {
                    mv[n] = *reinterpret_cast<const float4*>(mrow + n * 16);
                    mx.x = fmaxf(mx.x, mv[n].x); mx.y = fmaxf(mx.y, mv[n].y); mx.z = fmaxf(mx.z, mv[n].z); mx.w = fmaxf(mx.w, mv[n].w);
                }
                float4 den = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int n = 0; n < 9; ++n) {
                    mv[n].x = __expf(mv[n].x - mx.x); mv[n].y = __expf(mv[n].y - mx.y);
                    mv[n].z = __expf(mv[n].z - mx.z); mv[n].w = __expf(mv[n].w - mx.w);
                    den.x += mv[n].x; den.y += mv[n].y; den.z += mv[n].z; den.w += mv[n].w;
                }
                const float4 inv = make_float4(1.0f / den.x, 1.0f / den.y, 1.0f / den.z, 1.0f / den.w);
#pragma unroll
                for (int n = 0; n < 9; ++n) { mv[n].x *= inv.x; mv[n].y *= inv.y; mv[n].z *= inv.z; mv[n].w *= inv.w; }
                for (int pi = 0; pi < up.npred; ++pi) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const size_t plane = ((size_t)pi * up.B + b) * 2 + c;
                        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int n = 0; n < 9; ++n) {
                            const int y2 = y + n / 3 - 1, x2 = x + n % 3 - 1;
                            const float dv = (y2 >= 0 && y2 < up.h && x2 >= 0 && x2 < up.w) ? up.depth[plane * hw + (size_t)y2 * up.w + x2] : 0.f;
                            a.x += mv[n].x * dv; a.y += mv[n].y * dv; a.z += mv[n].z * dv; a.w += mv[n].w * dv;
                        }
                        *reinterpret_cast<float4*>(up.out + (plane * up.h * 4 + (size_t)y * 4 + i) * ((size_t)up.w * 4) + (size_t)x * 4) = a;
                    }
                }
            }
        }
        return;
    }
    if constexpr (!LAST) __syncthreads();                     // every wave is done reading the layer's input: overwrite it in place
    auto emit = [&](const f32x4_t& a, int n, int mrow) {
        const int ch = n * 16 + (lane >> 4) * 4;
        const int trow = mrow * 16 + (lane & 15);
        const float4 b4 = *reinterpret_cast<const float4*>(bias + ch);
        float v[4] = {a[0] + b4.x, a[1] + b4.y, a[2] + b4.z, a[3] + b4.w};
        if constexpr (!LAST) {
            uint32_t h01, l01, h23, l23;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = v[r] < 0.f ? 0.f : v[r];
            split_bf16x2(v[0], v[1], h01, l01); split_bf16x2(v[2], v[3], h23, l23);
            const int off = act_swz(trow, ch >> 3) + (ch & 7) * 2;              // 8 bytes: channels ch..ch+3
            *reinterpret_cast<uint2*>(act_hi + off) = make_uint2(h01, h23);
            *reinterpret_cast<uint2*>(act_lo + off) = make_uint2(l01, l23);
        } else {
            const long long row = row0 + trow;
            if constexpr (TAILN == 1) {
                if (up.npred < 0) {
                    // fused Gaussian update (models/MAGNET.py:60-69; gaussian_update_cl_kernel's arithmetic): channels 0, 1 of the head =
                    // the first quad's lanes; interior positions only
                    if (ch != 0 || row >= rows) return;
                    const int wp = up.w + 2, img_rows = (up.h + 2) * wp;
                    const int b = (int)((unsigned)row / (unsigned)img_rows);
                    const int rem = (int)((unsigned)row - (unsigned)b * (unsigned)img_rows);
                    const int yy = rem / wp, xx = rem - yy * wp;
                    if (yy < 1 || yy > up.h || xx < 1 || xx > up.w) return;
                    const size_t hw = (size_t)up.h * up.w, pp = (size_t)(yy - 1) * up.w + (xx - 1);
                    const float mu0 = up.depth[((size_t)b * 2 + 0) * hw + pp], sg0 = up.depth[((size_t)b * 2 + 1) * hw + pp];
                    const float mu1 = mu0 + (v[0] * sg0);
                    const float e = (v[1] > 0.f) ? v[1] : expm1f(v[1]);
                    up.out[((size_t)b * 2 + 0) * hw + pp] = mu1;
                    up.out[((size_t)b * 2 + 1) * hw + pp] = ((e + 1.0f) + 1e-10f) * sg0;
                    return;
                }
            }
            if (row < rows) *reinterpret_cast<float4*>(out + (size_t)row * out_ld + ch) = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int m = 0; m < MA; ++m) emit(acc[j][m], wv + NW * j, m);
    if constexpr (REM) {
#pragma unroll
        for (int m = 0; m < MR; ++m) emit(accr[m], NJ * NW, wv * MR + m);
    }
    if constexpr (!LAST) __syncthreads();
}

// One MFMA of the K loop.  SWAP (kernels with a fused tail): operands exchanged, so the accumulator holds C^T — a lane has 4
// consecutive output CHANNELS of one row, and the tail's activation tile is written with packed conversions and 8-byte LDS stores
// (the plain orientation gives 4 consecutive rows of one channel: 128 two-byte stores per lane and tile).
template <bool SWAP>
__device__ __forceinline__ f32x4_t cv_mma(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
    if constexpr (SWAP) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// The same for the single-plane fp16 format: a, b are fp16 fragments
template <bool SWAP>
__device__ __forceinline__ f32x4_t cv_mma_f16(const f16x8_t& a, const f16x8_t& b, const f32x4_t& c) {
    if constexpr (SWAP) return __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// The 16-byte fragment read (LDS or global): 8 bf16 / fp16 of one row's K slot
template <typename V = bf16x8_t>
__device__ __forceinline__ V ld_frag(const void* ptr) { return __builtin_bit_cast(V, *reinterpret_cast<const uint4*>(ptr)); }

// The step between a LOAD phase and the reads of what it waited for: all but the N newest DMA pieces of this wave have landed and its
// LDS reads have returned, then the workgroup barrier.
// FENCE: a trailing compiler fence, so that no LDS access is hoisted above the barrier (WIN == 2, 4 waves).
template <int N, bool FENCE = false>
__device__ __forceinline__ void wait_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (FENCE) asm volatile("" ::: "memory");
}

// Position of a staging stream in the K loop's step order (K chunk outer, `i` inner): i = tap row of a window stream, tap of a
// weight stream.  advance(n) steps to the next of the n inner positions and says whether it moved on to the next K chunk.
struct StepCounter {
    int i = 0, k0 = 0;
    __device__ __forceinline__ bool advance(int n) {
        const bool wrap = ++i == n;
        if (wrap) { i = 0; k0 += CV_BK; }
        return wrap;
    }
};

// LDS layout of the K loop's ring for one kernel instance.  conv_mfma_tile places its slots with these constants and launch_conv_nf
// asks for TOTAL bytes, so the launcher's byte count is the kernel's by construction (a mismatch would be an out-of-bounds LDS-DMA).
// A window slot is the [hi | lo] planes of AW_ROWS rows (a plain A tile: CV_BM rows); a weight slot the [hi | lo] planes of BN rows.
//   WIN == 0: 2*SPB stages of [window | weights], interleaved         WIN == 1: 2 window slots, then 2 weight slots
//   WIN == 2: 1 window slot, then a 3-slot weight ring
//   F16 (the single-plane fp16 format, WIN == 2 and WIN == 0): the same slots with ONE plane each — no lo plane behind the window or a weight tile
template <int NF, int WN, int BM, int SPB, int NT, bool PP, int WIN, bool F16 = false>
struct ConvLds {
    static_assert(!F16 || WIN == 2 || WIN == 0, "the single-plane fp16 format exists on the register-window loops and the windowless 4-wave loop");
    static_assert(!F16 || WIN == 2 || (!PP && NT == 256 && SPB == 1), "windowless fp16: the 4-wave / 2-slot loop");
    static constexpr int BN = NF * 16;
    static constexpr int AW_ROWS = WIN ? BM + 8 : BM;             // window: up to (3-1)*2 extra rows (dilation 2), padded to 8
    static constexpr int A_BYTES = AW_ROWS * CV_ROW, B_BYTES = BN * CV_ROW;       // one plane of a window / of a weight tile
    static constexpr int AW_BYTES = (F16 ? 1 : 2) * A_BYTES;                      // window slot
    static constexpr int BW_BYTES = (F16 ? 1 : 2) * B_BYTES;                      // weight slot
    static constexpr int A_SLOTS = WIN == 2 ? 1 : WIN == 0 ? 2 * SPB : 2;
    static constexpr int B_SLOTS = WIN == 2 ? 3 : 2 * SPB;
    static constexpr int A_STRIDE = WIN ? AW_BYTES : AW_BYTES + BW_BYTES;         // bytes from a window slot to the next
    static constexpr int B_STRIDE = WIN ? BW_BYTES : AW_BYTES + BW_BYTES;         // bytes from a weight slot to the next
    static constexpr int B_RING = WIN ? A_SLOTS * AW_BYTES : AW_BYTES;            // first weight slot
    static constexpr int RING_BYTES = A_SLOTS * AW_BYTES + B_SLOTS * BW_BYTES;
    static constexpr int EPI_BYTES = (NT / 64) * 16 * ((NF / WN) * 16 + 4) * 4;   // the plain epilogue's staging rows (SROW floats per row)
    static constexpr int TOTAL = RING_BYTES > EPI_BYTES ? RING_BYTES : EPI_BYTES;
};

// TAIL = 0: plain layer.  TAIL = 16-column fragments of the fused tail's last layer (1, 8 or 9): see ConvParams::tail_*.
// PP = "ping-pong" K loop: NT = 512 threads = 8 waves = two wave groups (waves 0-3 / 4-7: one wave of each group per SIMD) that
// run the same program half a K step apart — while one group issues its fragment reads and the LDS-DMA of the stage two steps
// ahead, the other owns the matrix pipe — with counted vmcnt waits and raw s_barriers (no DMA drain at a barrier); it exists with a
// row window only (WIN = 2).  The 4-wave / 2-slot loop (PP = false) drains the DMA queue (vmcnt(0)) at every step's
// __syncthreads and relies on a second workgroup per CU to fill the gap: 41 % of the matrix pipe; see DESIGN.md §4.3.
// WIN = row-window K loop: the taps of one tap ROW (ty fixed, tx = 0..tap_n-1) read the same activation rows shifted by tap_sx, so
// their A operand is staged ONCE per (K chunk, ty) as a window of CV_BM + (tap_n-1)*tap_sx rows and the tx sub-steps read their
// fragments at a row offset; only the weight tile changes per sub-step.  L2 requests per 3x3 tap row: 272 + 3*256 instead of
// 3*(256 + 256).  WIN = 1: two window slots + two weight slots in LDS, one flat loop over the sub-steps (2x2 taps).
// WIN = 2 (3x3 layers, default): the window's fragments for all three tx are held in registers, one window slot + a 3-slot weight
// ring with counted vmcnt waits (prefetch distance 2).
// __launch_bounds__(NT, 2): two waves per SIMD is what the LDS budget allows anyway, and with <= 256 registers hipcc selects the
// VGPR form of the MFMAs — with the default bound it kept the accumulators in AGPRs and moved all 64 of them through VGPRs
// (64 v_accvgpr_read + 64 v_accvgpr_write) on every trip of the K loop.
// One output tile (CV_BM rows x BN channels).  `bid` of `n_tiles`: the tile's position in launch order (the block id); `by`: the channel
// block.  A tile is CV_BM consecutive rows of the flattened (B, h+2, w+2) buffer.  Flat tiling cuts the whole buffer into tiles; per-image
// tiling (ConvParams::tiles_per_img, the launches with a fused Gaussian update / upsampling) cuts each image's h * wp rows from its first
// interior image row on, so the top and bottom border image rows — which no consumer reads — get no tile, and 64 frames of 120x160
// are 64 x 76 = 4 864 tiles = 19 full rounds of 256 workgroups instead of 4 941 = 19.3 (profiles/r8/NOTES.md).  Measured and not kept (the source is in the history): the ping-pong loop without a window (equal to the 4-wave loop, 5.83 vs
// 5.91 ms per C2 step), with a 2-slot LDS window, with fragment double-buffering and with deeper prefetch (4 % slower: 2.19 vs 2.10 ms,
// profiles/r4/conv_deeper_prefetch_vs_round3.log); persistent workgroups (0.7 % slower, profiles/r4/conv_persistent_ab.log); the 32x32x16 MFMA shape (5.5 %
// slower, profiles/r5/conv_m32_ab.log); a row-owned fused tail (see tail_layer_cols).
// F16 = the single-plane fp16 operand format (magnet_conv_mfma_f16): in_hi / w_hi are fp16 planes and there is no lo plane, so the
// staging blocks issue the hi pieces only and the two F16 loops below (copies of the WIN == 2 schedules) issue one
// v_mfma_f32_16x16x32_f16 per fragment pair; everything behind the K loop is the code of the bf16x3 instances.
// F16P = "plane to plane" (magnet_conv_mfma_f16p, the F-Net): F16 operands, and in the plain epilogue the residual input is ONE fp16
// plane (add_hi) and out_mode 3 writes ONE fp16 plane (out_hi).  Besides the two WIN == 2 loops it runs the windowless loop at the
// bottom with one fp16 MFMA per fragment pair (taps 1 and 4), and the 4-wave WIN == 2 loop at BN = 32 (one weight piece per wave).
// The decoder's wide instances (magnet_conv_mfma_f16d, the D-Net's plain layers) are F16 && F16P at 128 rows x 128 channels with
// gridDim.y = cout_pad / 128 channel blocks: the same two loops (WIN == 2 for 3x3, WIN == 0 for 1x1); their epilogue also takes LeakyReLU
// and the split-bf16 output (out_mode 0), which this template serves for every plain instance.
// SPLITK = the split-K form (magnet_conv_mfma_splitk; on fp16 planes magnet_conv_mfma_f16d_splitk): workgroup sk_z of sk_n runs the K loop over the input-channel chunks
// [floor(sk_z C / sk_n), floor((sk_z + 1) C / sk_n)) of the C = cin / 32 chunks, all taps — the chunk range, the activation channel offset
// and the weight offset change (the weight row pitch stays cin); the step order and the ring schedule are the plain loop's — and stores
// its raw fp32 accumulator tile to sk_work[sk_z][row][cout_pad], rows < p.rows: no bias, activation or border logic (the reduce kernel's).
// A partial therefore holds, to the bit, what the plain instance writes to out_f32 for that channel range alone with a zero bias.
template <int NF, int WN, int CV_BM, int SPB, int TAIL, int NT, bool PP, int WIN, bool F16 = false, bool F16P = false, bool SPLITK = false, bool NCHW = false>
__device__ __forceinline__ void conv_mfma_tile(const ConvParams& p, const unsigned bid, const unsigned n_tiles, const unsigned by, const int tid,
                                               [[maybe_unused]] float* __restrict__ sk_work = nullptr, [[maybe_unused]] const unsigned sk_z = 0,
                                               [[maybe_unused]] const unsigned sk_n = 1, [[maybe_unused]] const ConvSrc nchw = ConvSrc{nullptr, 0}) {
#if defined(__HIP_DEVICE_COMPILE__)   // the buffer-descriptor builtins do not exist in the host pass (which only needs the stub)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // the K loop's ring (ConvLds; declared here, not passed in: a pointer
                                                                            // parameter is a generic pointer, and its casts to LDS pointers get null checks)
    using L = ConvLds<NF, WN, CV_BM, SPB, NT, PP, WIN, F16>;
    static_assert(!F16P || (F16 && TAIL == 0 && !PP), "plane to plane: fp16 operands, plain epilogue, 4 waves");
    static_assert(!SPLITK || ((!F16 || F16P) && TAIL == 0 && !PP && NT == 256 && (WIN == 2 || WIN == 0)),
                  "split-K: the two 4-wave loops (bf16x3, or fp16 plane to plane), no tail");
    constexpr int BN = L::BN, A_BYTES = L::A_BYTES, B_BYTES = L::B_BYTES;
    constexpr int RP = NT / 4;                      // tile rows filled by one DMA instruction per wave set (4 lanes per 64-byte row)
    constexpr int A_PT = CV_BM / RP;                           // 16-byte vectors per thread per A plane (1, 2 or 4)
    constexpr int WM = (NT / 64) / WN;                // waves along M
    constexpr int MF = CV_BM / (WM * 16);             // M fragments per wave (2 or 4; 64-row tile: 2x2 waves of 32 rows)
    constexpr int NFW = NF / WN;                      // N fragments per wave
    static_assert(NF % WN == 0, "N fragments must split evenly over the waves");
    const int lane = tid & 63, wv = tid >> 6;
    const int wm = wv / WN, wn = wv % WN;
    // XCD-aware tile order: hardware deals consecutive block ids round-robin to the 8 XCDs; remap so each XCD (one
    // private L2) owns a contiguous run of row tiles — vertically adjacent tiles share their halo rows (bijective).
    long long tile_id;
    {
        const unsigned n = n_tiles, q = n / 8, r = n % 8, xcd = bid % 8, idx = bid / 8;
        tile_id = (long long)((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    // tile -> first row.  Flat: tile t starts at row t * BM.  Per image (ConvParams::tiles_per_img, chosen by launch_conv_nf): tile t of
    // image i starts at the image's first interior image row + t * BM.  Either way the tile is the CV_BM consecutive flat rows from
    // row0 on, so nothing below depends on the form; bid is wave-uniform, so the division runs once per workgroup on the scalar unit
    long long row0 = tile_id * CV_BM;
    if (p.tiles_per_img) {
        const unsigned img = (unsigned)tile_id / (unsigned)p.tiles_per_img, t = (unsigned)tile_id - img * (unsigned)p.tiles_per_img;
        row0 = (long long)img * ((p.up_h + 2) * p.wp) + p.wp + (long long)t * CV_BM;
    }
    const int n0 = by * BN;

    // staging by LDS-DMA (global_load_lds_dwordx4: global -> LDS without a VGPR round trip or ds_write): a
    // 64-byte K-slice of one row = 4 x 16 B; thread -> (row = tid>>2 (+64, +128 ...), physical slot = tid&3).  The DMA
    // writes lane-linearly (wave-uniform base + lane*16), so the XOR swizzle is applied to the SOURCE: the lane
    // that fills physical slot ps of row r fetches logical K slot ps ^ ((r>>1)&3)  (cdna_hip_programming.md rule 21).
    constexpr int B_PT = (BN + RP - 1) / RP;                   // 16-byte vectors per thread per B plane
    // split-K: this workgroup's chunks [sk_c0, sk_c0 + ksteps_per_tap) of the cin / 32
    [[maybe_unused]] const int sk_c0 = SPLITK ? (int)((long long)sk_z * (p.cin / CV_BK) / sk_n) : 0;
    const int ksteps_per_tap = [&] {
        if constexpr (SPLITK) return (int)((long long)(sk_z + 1) * (p.cin / CV_BK) / sk_n) - sk_c0;
        else return p.cin / CV_BK;
    }();
    const int nsteps = p.taps * ksteps_per_tap;
    const int st_r = tid >> 2, st_q = tid & 3;
    const int st_k = (st_q ^ ((st_r >> 1) & 3)) * 8;          // logical K offset (elements) this lane fetches (cv_swz)
    const int wave_row = __builtin_amdgcn_readfirstlane(wv * 16);   // first tile row this wave's DMA instruction fills

    // step order: K-chunk outer, tap inner — the 9 taps of one 32-channel chunk re-read (shifted) the same 64-byte
    // row slices back to back, a working set of ~50 KB per workgroup that stays in the XCD's L2; tap-major order
    // swept 164 KB per workgroup between re-reads (x64 resident workgroups >> 4 MiB L2).
    //
    // Addressing: buffer descriptors (wave-uniform SGPRs) + one 32-bit per-lane byte offset.  The activation descriptor
    // covers exactly the row window this workgroup can touch, [row0 + min tap offset, row0 + BM + max tap offset) cut to
    // [0, rows): a row outside it is out of range for the hardware bounds check and reads as zero — no per-lane
    // clamping, no 64-bit per-lane arithmetic (the first version spent 137 VALU + 85 SALU instructions per K step
    // next to 48 MFMAs, mostly on this; such rows only ever feed border / guard outputs).  Per step and DMA piece:
    // one v_add of a scalar.
    static_assert(SPB == 1, "the step counters below assume one K stage per barrier interval");
    long long base_row = row0 + p.min_off;  base_row = base_row < 0 ? 0 : base_row;
    long long end_row = row0 + CV_BM + p.max_off;  end_row = end_row > p.rows ? p.rows : end_row;
    const uint32_t flags = 0x00020000u;
    const __amdgpu_buffer_rsrc_t ra_hi = __builtin_amdgcn_make_buffer_rsrc((void*)(p.in_hi + base_row * p.in_ld), 0,
                                                                           (int)((end_row - base_row) * p.in_ld * 2), flags);
    const __amdgpu_buffer_rsrc_t ra_lo = __builtin_amdgcn_make_buffer_rsrc((void*)((F16 ? p.in_hi : p.in_lo) + base_row * p.in_ld), 0,
                                                                           (int)((end_row - base_row) * p.in_ld * 2), flags);
    const int w_bytes = p.taps * p.cout_pad * p.cin * 2;
    const __amdgpu_buffer_rsrc_t rb_hi = __builtin_amdgcn_make_buffer_rsrc((void*)p.w_hi, 0, w_bytes, flags);
    const __amdgpu_buffer_rsrc_t rb_lo = __builtin_amdgcn_make_buffer_rsrc((void*)(F16 ? p.w_hi : p.w_lo), 0, w_bytes, flags);   // F16: never used
    int a_v[A_PT], b_v[B_PT];                                  // per-lane byte offsets, constant over the K loop
#pragma unroll
    for (int i = 0; i < A_PT; ++i) a_v[i] = (((int)(row0 - base_row) + st_r + i * RP) * p.in_ld + st_k) * 2;
#pragma unroll
    for (int i = 0; i < B_PT; ++i) b_v[i] = ((n0 + st_r + i * RP) * p.cin + st_k) * 2;
    typedef void __attribute__((address_space(3)))* lptr_t;
#define CV_BLDS(rsrc, lp, voff) __builtin_amdgcn_raw_ptr_buffer_load_lds((rsrc), (lptr_t)(lp), 16, (voff), 0, 0, 0)
    // ---- the building blocks of every K loop below; the loops differ in their schedule only ----
    auto win_slot = [&](int s) { return smem + s * L::A_STRIDE; };                  // ConvLds: the layout
    auto wt_slot = [&](int s) { return smem + L::B_RING + s * L::B_STRIDE; };
    // wave-uniform byte offset of the window (or plain A tile) of tap (ty, tx), K chunk from k0 on.  (The weight tile's offset,
    // (tap * cout_pad * cin + k0) * 2, is spelled at its stage_weights calls: in a helper that takes `tap` by value the compiler
    // associates the product the other way round and every prologue changes.)
    auto a_step = [&](int ty, int tx, int k0) { return (((ty + p.tap_o0) * p.tap_sy + (tx + p.tap_o0) * p.tap_sx) * p.in_ld + k0) * 2; };
    // hi / lo DMA pieces of a row window of `aw` rows into the slot at sa_hi; the aw - CV_BM rows past the tile are a few lanes of wave 0
    // (two more pieces for its counted waits).  A plain A tile is a window of CV_BM rows.
    auto stage_window = [&](unsigned char* sa_hi, const int a_u, const int aw) {
        [[maybe_unused]] unsigned char* sa_lo = sa_hi + A_BYTES;
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            CV_BLDS(ra_hi, sa_hi + (wave_row + i * RP) * CV_ROW, a_v[i] + a_u);
            if constexpr (!F16) CV_BLDS(ra_lo, sa_lo + (wave_row + i * RP) * CV_ROW, a_v[i] + a_u);
        }
        if constexpr (WIN != 0) {
            if (wv == 0 && st_r < aw - CV_BM) {
                const int ax = a_v[0] + CV_BM * p.in_ld * 2;
                CV_BLDS(ra_hi, sa_hi + CV_BM * CV_ROW, ax + a_u);
                if constexpr (!F16) CV_BLDS(ra_lo, sa_lo + CV_BM * CV_ROW, ax + a_u);
            }
        }
    };
    // hi / lo DMA pieces of a weight tile; the last row pass is partial only where BN is no multiple of the rows of a pass
    auto stage_weights = [&](unsigned char* sb_hi, unsigned char* sb_lo, const int b_u) {
#pragma unroll
        for (int i = 0; i < B_PT; ++i) {
            if constexpr (BN % RP != 0) {
                if (st_r + i * RP >= BN) continue;
            }
            CV_BLDS(rb_hi, sb_hi + (wave_row + i * RP) * CV_ROW, b_v[i] + b_u);
            if constexpr (!F16) CV_BLDS(rb_lo, sb_lo + (wave_row + i * RP) * CV_ROW, b_v[i] + b_u);
        }
    };

    f32x4_t acc[MF][NFW];
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
        for (int n = 0; n < NFW; ++n) acc[m][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // fused-tail kernels (C^T accumulators: 4 consecutive channels of one row per lane): the loop-invariant partial sums of the
    // hoisted G-Net layer (ConvParams::addend) are the accumulators' INITIAL value — sixteen 16-byte loads whose latency hides
    // behind the K loop's prologue instead of sitting exposed in the epilogue (the short K = 288 / 576 per-iteration layers)
    if constexpr (TAIL > 0) {
        if (p.addend) {
#pragma unroll
            for (int m = 0; m < MF; ++m)
#pragma unroll
                for (int n = 0; n < NFW; ++n) {
                    const long long row = row0 + wm * (MF * 16) + m * 16 + (lane & 15);
                    const int ch = wn * (NFW * 16) + n * 16 + (lane >> 4) * 4;
                    const float4 a4 = *reinterpret_cast<const float4*>(p.addend + (size_t)(row < p.rows ? row : p.rows - 1) * p.addend_ld + ch);
                    acc[m][n] = f32x4_t{a4.x, a4.y, a4.z, a4.w};
                }
        }
    }

    // fragment addressing: lane -> (row/col = lane & 15, K slot = lane >> 4); every fragment's first row is a
    // multiple of 16, so the swizzle term depends on the lane only
    const int frow = lane & 15;
    const int a_off = cv_swz(wm * (MF * 16) + frow, lane >> 4);       // + m*16*CV_ROW
    const int b_off = cv_swz(wn * (NFW * 16) + frow, lane >> 4);      // + n*16*CV_ROW

    // fragment rows of a window shifted by tx*tap_sx: the swizzle term follows the ACTUAL LDS row, so one offset per tx
    int a_offx[3];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) a_offx[tx] = cv_swz(wm * (MF * 16) + frow + tx * p.tap_sx, lane >> 4);

    // the split product of one fragment column n: term-major order — consecutive MFMAs write DIFFERENT accumulators (a dependent
    // MFMA on the same accumulator waits out the full pipeline latency); small terms first
    auto mma3 = [&](const int n, const bf16x8_t (&ah)[MF], const bf16x8_t (&al)[MF], const bf16x8_t bh, const bf16x8_t bl) {
#pragma unroll
        for (int m = 0; m < MF; ++m) acc[m][n] = cv_mma<(TAIL > 0)>(al[m], bh, acc[m][n]);
#pragma unroll
        for (int m = 0; m < MF; ++m) acc[m][n] = cv_mma<(TAIL > 0)>(ah[m], bl, acc[m][n]);
#pragma unroll
        for (int m = 0; m < MF; ++m) acc[m][n] = cv_mma<(TAIL > 0)>(ah[m], bh, acc[m][n]);
    };
    // fragment reads of a weight slot's NFW columns
    auto load_b = [&](const unsigned char* sb_hi, bf16x8_t (&fbh)[NFW], bf16x8_t (&fbl)[NFW]) {
#pragma unroll
        for (int n = 0; n < NFW; ++n) {
            fbh[n] = ld_frag(sb_hi + b_off + n * 16 * CV_ROW);
            fbl[n] = ld_frag(sb_hi + B_BYTES + b_off + n * 16 * CV_ROW);
        }
    };
    // one K stage of MFMAs: window (or A tile) slot at sa_hi read at fragment offset a_of, weight slot at sb_hi
    auto compute = [&](const unsigned char* sa_hi, const unsigned char* sb_hi, const int a_of) {
        bf16x8_t ah[MF], al[MF];
#pragma unroll
        for (int m = 0; m < MF; ++m) {
            ah[m] = ld_frag(sa_hi + a_of + m * 16 * CV_ROW);
            al[m] = ld_frag(sa_hi + A_BYTES + a_of + m * 16 * CV_ROW);
        }
#pragma unroll
        for (int n = 0; n < NFW; ++n) mma3(n, ah, al, ld_frag(sb_hi + b_off + n * 16 * CV_ROW), ld_frag(sb_hi + B_BYTES + b_off + n * 16 * CV_ROW));
    };

    // the same for the single-plane fp16 format: one MFMA per fragment pair
    [[maybe_unused]] auto compute16 = [&](const unsigned char* sa, const unsigned char* sb, const int a_of) {
        f16x8_t ah[MF];
#pragma unroll
        for (int m = 0; m < MF; ++m) ah[m] = ld_frag<f16x8_t>(sa + a_of + m * 16 * CV_ROW);
#pragma unroll
        for (int n = 0; n < NFW; ++n) {
            const f16x8_t fb = ld_frag<f16x8_t>(sb + b_off + n * 16 * CV_ROW);
#pragma unroll
            for (int m = 0; m < MF; ++m) acc[m][n] = cv_mma_f16<(TAIL > 0)>(ah[m], fb, acc[m][n]);
        }
    };

    if constexpr (F16 && PP) {
        // ---- single-plane fp16, 8 waves: the ping-pong x register-window schedule below with one DMA piece where it has a (hi, lo)
        // pair — BP = B_PT, AP = A_PT, one extra window piece for wave 0 — 12 + 4 fragment reads per group / sub-step instead of 24 + 8,
        // and 16 MFMAs per compute phase instead of 48.  Same phase order, same RAW / WAR argument.
        static_assert(WIN == 2 && NT == 512 && SPB == 1 && BN % RP == 0 && CV_BM % RP == 0, "8 waves, whole DMA passes");
        constexpr int BP = B_PT, AP = A_PT;
        const int aw = CV_BM + 2 * p.tap_sx;
        const int ngroups = 3 * ksteps_per_tap;
        StepCounter gw, bs;                                   // next window (i = ty) / weight tile (i = tap) to fetch
        auto dma_a = [&]() { stage_window(win_slot(0), a_step(gw.i, 0, gw.k0), aw); gw.advance(3); };
        auto dma_b = [&](int slot) { stage_weights(wt_slot(slot), nullptr, (bs.i * p.cout_pad * p.cin + bs.k0) * 2); bs.advance(9); };
        f16x8_t ah[3][MF], fbh[NFW];
        auto load_b = [&](const unsigned char* sb) {
#pragma unroll
            for (int n = 0; n < NFW; ++n) fbh[n] = ld_frag<f16x8_t>(sb + b_off + n * 16 * CV_ROW);
        };
        auto mfmas = [&](const f16x8_t (&x)[MF]) {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int n = 0; n < NFW; ++n)
#pragma unroll
                for (int m = 0; m < MF; ++m) acc[m][n] = cv_mma_f16<(TAIL > 0)>(x[m], fbh[n], acc[m][n]);
            __builtin_amdgcn_s_setprio(0);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
        };
        const int grp = __builtin_amdgcn_readfirstlane(wv >> 2);
        dma_a();
        dma_b(0);
        dma_b(1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BP) : "memory");                 // window 0 and stage 0 landed (this wave's pieces)
        __builtin_amdgcn_s_barrier();
        if (grp == 1) __builtin_amdgcn_s_barrier();           // group 1 runs one barrier (= half a sub-step) behind group 0
        for (int g = 0; g < ngroups; ++g) {
            const bool lastg = g + 1 == ngroups;
            // ---- tx = 0 ----
            asm volatile("" ::: "memory");
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                for (int m = 0; m < MF; ++m) ah[tx][m] = ld_frag<f16x8_t>(win_slot(0) + a_offx[tx] + m * 16 * CV_ROW);
            load_b(wt_slot(0));
            dma_b(2);                                         // stage 3g + 2
            wait_barrier<BP>();                               // stage 3g + 1 landed
            mfmas(ah[0]);
            // ---- tx = 1 ----
            asm volatile("" ::: "memory");
            load_b(wt_slot(1));
            if (!lastg) {
                dma_b(0); dma_a();                            // stage 3g + 3, window g + 1
                if (wv == 0) wait_barrier<BP + AP + 1>(); else wait_barrier<BP + AP>();      // stage 3g + 2 landed
            } else wait_barrier<0>();
            mfmas(ah[1]);
            // ---- tx = 2 ----
            asm volatile("" ::: "memory");
            load_b(wt_slot(2));
            if (!lastg) { dma_b(1); wait_barrier<BP>(); }     // stage 3g + 4; stage 3g + 3 and window g + 1 landed
            else wait_barrier<0>();
            mfmas(ah[2]);
        }
        if (grp == 0) __builtin_amdgcn_s_barrier();           // balance group 1's extra barrier
        __syncthreads();                                      // nothing in flight; the ring is dead
    } else
    if constexpr (F16 && WIN == 2) {
        // ---- single-plane fp16, 4 waves: the register-window loop below (prefetch distance 2, slot tx holds stage 3g + tx) with one
        // DMA piece per (hi, lo) pair; the window is 48 registers instead of 96
        // BN = 32 (F-Net's 32-wide trunk): the weight tile is 32 rows x 64 B = half a row pass; wave w stages rows 8 w .. 8 w + 7 with
        // its lanes 0 .. 31 — ONE piece per wave, so the counted waits stay wave-uniform (as a row pass waves 2 and 3 had nothing to count)
        static_assert(!PP && SPB == 1 && NT == 256 && (BN % RP == 0 || BN == 32), "window loop with register-resident A: 4 waves, whole DMA passes (or the 32-wide case)");
        constexpr int BP = B_PT, AP = A_PT;
        static_assert(BN != 32 || BP == 1, "32-wide: one weight piece per wave and stage");
        const int aw = CV_BM + 2 * p.tap_sx;
        const int ngroups = 3 * ksteps_per_tap;               // (K chunk, ty) pairs, ty inner
        StepCounter gw, bs;
        if constexpr (SPLITK) gw.k0 = bs.k0 = sk_c0 * CV_BK;  // the range's first channel (magnet_conv_mfma_f16d_splitk), as in the bf16x3 loop below
        auto dma_a = [&]() { stage_window(win_slot(0), a_step(gw.i, 0, gw.k0), aw); gw.advance(3); };
        // BN = 32: row 8 w + (lane >> 2) of the tile; 8 w is a multiple of 8, so the swizzle term of st_k (from row 16 w + (lane >> 2)) is this row's
        [[maybe_unused]] const int b_v32 = ((n0 + (wave_row >> 1) + (lane >> 2)) * p.cin + st_k) * 2;
        auto dma_b = [&](int slot) {
            const int b_u = (bs.i * p.cout_pad * p.cin + bs.k0) * 2;
            if constexpr (BN == 32) {
                if (lane < 32) CV_BLDS(rb_hi, wt_slot(slot) + (wave_row >> 1) * CV_ROW, b_v32 + b_u);
            } else stage_weights(wt_slot(slot), nullptr, b_u);
            bs.advance(9);
        };
        f16x8_t ah[3][MF];
        auto mfma_b = [&](int slot, const f16x8_t (&x)[MF]) {
            f16x8_t fbh[NFW];
#pragma unroll
            for (int n = 0; n < NFW; ++n) fbh[n] = ld_frag<f16x8_t>(wt_slot(slot) + b_off + n * 16 * CV_ROW);
#pragma unroll
            for (int n = 0; n < NFW; ++n)
#pragma unroll
                for (int m = 0; m < MF; ++m) acc[m][n] = cv_mma_f16<(TAIL > 0)>(x[m], fbh[n], acc[m][n]);
        };
        dma_a();
        dma_b(0);
        dma_b(1);
        for (int g = 0; g < ngroups; ++g) {
            const bool lastg = g + 1 == ngroups;
            // ---- tx = 0: stage 3g (slot 0) and window g have landed; refill slot 2 with stage 3g + 2 ----
            wait_barrier<BP, true>();
            dma_b(2);
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                for (int m = 0; m < MF; ++m) ah[tx][m] = ld_frag<f16x8_t>(win_slot(0) + a_offx[tx] + m * 16 * CV_ROW);
            mfma_b(0, ah[0]);
            // ---- tx = 1: every wave holds window g in registers (lgkmcnt(0) before the barrier): fetch window g + 1 ----
            wait_barrier<BP, true>();
            if (!lastg) { dma_b(0); dma_a(); }
            mfma_b(1, ah[1]);
            // ---- tx = 2 (the window's pieces, issued after the weight pieces, stay in flight; wave 0's extra piece makes its wait
            // the stricter by one piece of stage 3g + 3, never the looser) ----
            if (!lastg) { wait_barrier<BP + AP, true>(); dma_b(1); }
            else wait_barrier<0, true>();
            mfma_b(2, ah[2]);
        }
        __syncthreads();                                      // nothing in flight; the ring is dead (the epilogue reuses it)
    } else
    if constexpr (WIN == 2 && PP) {
        // ---- ping-pong x register window (DEFAULT for 128-wide 3x3 layers): 256-row tile, two wave groups half a step apart as in the PP
        // loop below, but the LOAD phase of a sub-step is only the 8 weight-fragment reads (+ the 24 window reads once per group)
        // and ~3.4 DMA pieces per wave, so it fits under the other group's 48 MFMAs.  Phase order per group: L_s = reads of stage
        // s, DMA of stage s+2 (and of window g+1 at tx = 1), counted vmcnt for everything older, lgkmcnt(0), barrier; C_s = MFMAs,
        // barrier.  RAW: a stage is read one L phase after every wave's wait for it and a barrier both groups passed; WAR: a
        // slot is refilled in the L phase after the one whose reads of it retired before a barrier both groups passed.
        static_assert(NT == 512 && SPB == 1 && BN % RP == 0 && CV_BM % RP == 0, "8 waves, whole DMA passes");
        constexpr int BP = 2 * B_PT, AP = 2 * A_PT;
        const int aw = CV_BM + 2 * p.tap_sx;
        const int ngroups = 3 * ksteps_per_tap;
        StepCounter gw, bs;                                   // next window (i = ty) / weight tile (i = tap) to fetch
        auto dma_a = [&]() { stage_window(win_slot(0), a_step(gw.i, 0, gw.k0), aw); gw.advance(3); };
        auto dma_b = [&](int slot) { stage_weights(wt_slot(slot), wt_slot(slot) + B_BYTES, (bs.i * p.cout_pad * p.cin + bs.k0) * 2); bs.advance(9); };
        bf16x8_t ah[3][MF], al[3][MF], fbh[NFW], fbl[NFW];
        auto load_win = [&]() {                               // window g -> registers, all three tx
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                for (int m = 0; m < MF; ++m) {
                    ah[tx][m] = ld_frag(win_slot(0) + a_offx[tx] + m * 16 * CV_ROW);
                    al[tx][m] = ld_frag(win_slot(0) + A_BYTES + a_offx[tx] + m * 16 * CV_ROW);
                }
        };
        auto mfmas = [&](const bf16x8_t (&xh)[MF], const bf16x8_t (&xl)[MF]) {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int n = 0; n < NFW; ++n) mma3(n, xh, xl, fbh[n], fbl[n]);
            __builtin_amdgcn_s_setprio(0);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
        };
        const int grp = __builtin_amdgcn_readfirstlane(wv >> 2);
        if constexpr (NCHW) {
            // ---- the same loop with the K chunks k0 >= nchw.c0 taken from nchw.ptr, (B, cin - c0, h, w) fp32 (magnet_conv_mfma_nchw):
            // the window of such a (chunk, ty) is not DMA'd from the (hi, lo) planes.  Wave wv owns window rows 32 wv .. 32 wv + 31
            // (wave 7 also rows 256, 257).  Per-image tiling is in effect, so those consecutive padded rows are ONE run of consecutive
            // pixels of the tile's image (the border columns are simply absent from it).  FETCH: the wave copies that run, for the
            // chunk's 32 channels, into its own fp32 staging area [32 channels][40 floats] by NP = 5 LDS-DMA pieces of 64 x 16 bytes;
            // a channel's run starts at its first pixel's address rounded down to 16 bytes (<= 34 pixels + 3 <= 40).  CONVERT, two
            // sub-steps later: lane item = (window row, 16-byte slot) as in stage_window — 8 ds_read_b32, split_bf16x2 as the pack
            // does, and ds_write_b128 of hi and lo to the swizzled position the plane DMA would have filled; border positions and rows
            // outside the image's padded grid read a zeroed area instead and become 16 zero bytes in both planes.  A wave converts
            // only what it fetched itself, so the counted vmcnt orders the two and the staging area needs no barrier.
            // The staging area is LDS the launch owns anyway (the fused tail's 128 KB) behind the ring.  Staging order of the channels:
            // channel 8 ql + i sits at index 4 i + ql, so the four 8-channel slots of a row read banks 40 apart (= 8 mod 32) and the
            // eight rows of a ds_read_b32 lane group consecutive ones: conflict-free.
            // Schedule: FETCH of window g + 1 in the tx = 0 L phase behind dma_b(2); CONVERT split over the tx = 1 L phase (behind
            // dma_b(0) and vmcnt(BP): the wave's first 16 rows) and the tx = 2 L phase (the rest) — the two phases in which the plane
            // DMA's bytes land today: WAR (both groups' load_win retired behind a barrier both passed) and RAW (lgkmcnt(0) and the L
            // phase's barrier before the next load_win) hold as they do for the DMA.  (All of it in the tx = 2 phase: that phase
            // outgrew the other group's MFMA phase, each launch +9 %; profiles/xd3_nchw/NOTES.md.)
            static_assert(TAIL > 0 && CV_BM == 256 && A_PT == 2 && B_PT == 1, "the fp32-source form exists for the 256-row fused-tail instances");
            constexpr int NP = 5, ST_WAVE = NP * 1024, ST_BASE = L::RING_BYTES, ZERO_BASE = ST_BASE + 8 * ST_WAVE, ZERO_BYTES = 4608;
            static_assert(ZERO_BASE + ZERO_BYTES <= CV_BM * 512, "staging fits the fused tail's LDS request");
            static_assert(ZERO_BYTES >= 7 * 640 + 16, "a zero read at every channel offset");
            const int h = p.up_h, w = p.up_w, hw = h * w, hwm = hw & 3;
            const unsigned img = (unsigned)tile_id / (unsigned)p.tiles_per_img, t_in = (unsigned)tile_id - img * (unsigned)p.tiles_per_img;
            const int src_C = p.cin - nchw.c0;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(nchw.ptr + (size_t)img * src_C * hw), 0, src_C * hw * 4, flags);
            // window row r of tap row ty is position e + ty * wp of the image's padded grid, e = 256 t - 1 + r (>= -1)
            const int e_w = __builtin_amdgcn_readfirstlane((int)t_in * CV_BM - 1 + wv * 32);
            const int n_ys = (int)((unsigned)(e_w + p.wp) / (unsigned)p.wp) - 1, n_xs = e_w - n_ys * p.wp;
            const int n_xcl = n_xs - 1 < 0 ? 0 : (n_xs - 1 > w ? w : n_xs - 1);     // interior pixels of the run's first image row before it
            int f_cl[NP], f_j[NP];                                                  // fetch item -> channel * hw, 4-pixel group
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) {
                const int it = pc * 64 + lane, idx = it / 10;
                f_j[pc] = it - idx * 10;
                f_cl[pc] = ((idx & 3) * 8 + (idx >> 2)) * hw;
            }
            const int ql = (lane & 3) ^ ((lane >> 3) & 3);                          // logical K slot of this lane's physical slot (cv_swz)
            int c_y[3], c_lb[3];                                                    // convert item -> image row at ty = 0, staging byte offset at pix0 = 0
#pragma unroll
            for (int ps = 0; ps < 3; ++ps) {
                const int e = (int)t_in * CV_BM - 1 + (ps < 2 ? wv * 32 + ps * 16 : CV_BM) + (lane >> 2);
                const int y = (int)((unsigned)(e + p.wp) / (unsigned)p.wp) - 1, x = e - y * p.wp;
                c_y[ps] = (x >= 1 && x <= w) ? y : -(1 << 20);
                c_lb[ps] = ST_BASE + wv * ST_WAVE + ql * 160 + ((y - 1) * w + x - 1) * 4;
            }
            // first pixel of the wave's run at tap row ty, then the pieces; returns that pixel
            auto fetch = [&](const int ty, const int k0) {
                const int yp = n_ys + ty;
                const int pix0 = yp < 1 ? 0 : (yp > h ? hw : (yp - 1) * w + n_xcl);
                const int u = (k0 - nchw.c0) * hw + pix0;
#pragma unroll
                for (int pc = 0; pc < NP; ++pc)
                    CV_BLDS(rs, smem + ST_BASE + wv * ST_WAVE + pc * 1024, (((f_cl[pc] + u) >> 2) + f_j[pc]) << 4);
                return pix0;
            };
            // part 1: the wave's first 16 rows; part 2: its other 16 (and wave 7's two extra rows)
            auto convert = [&](const int ty, const int pix0, const int part) {
                const int uc = (ty * w - pix0) * 4;
                int so[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) so[i] = i * 640 + (((pix0 + (i & 3) * hwm) & 3) << 2);
                auto pass = [&](const int cy, const int lb, unsigned char* dst) {
                    const int base = (unsigned)(cy + ty - 1) < (unsigned)h ? lb + uc : ZERO_BASE;
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const float*>(smem + base + so[i]);
                    uint32_t hh[4], ll[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {             // split_bf16x2 with its two subtractions spelled as statements: as plain
                        // C++ hipcc pairs them into one v_pk_add_f32 (half rate) behind four v_mov into aligned register pairs, and this
                        // phase's VALU time is MFMA time of the other wave group (profiles/xd3_nchw/NOTES.md)
                        hh[k] = f32x2_to_bf16x2_rne(v[2 * k], v[2 * k + 1]);
                        float d0, d1;
                        asm("v_sub_f32 %0, %1, %2" : "=v"(d0) : "v"(v[2 * k]), "v"(hh[k] << 16));
                        asm("v_sub_f32 %0, %1, %2" : "=v"(d1) : "v"(v[2 * k + 1]), "v"(hh[k] & 0xffff0000u));
                        ll[k] = f32x2_to_bf16x2_rne(d0, d1);
                    }
                    // stores as statements: before a store hipcc can see it drains every LDS-DMA piece in flight (vmcnt(0)), the two
                    // weight stages included; the L phase's own lgkmcnt(0) covers them
                    typedef uint32_t __attribute__((ext_vector_type(4))) u32x4_t;
                    const u32x4_t vh = {hh[0], hh[1], hh[2], hh[3]}, vl = {ll[0], ll[1], ll[2], ll[3]};
                    asm volatile("ds_write_b128 %0, %1\n\tds_write_b128 %0, %2 offset:%3"
                                 :: "v"((uint32_t)(uintptr_t)(lptr_t)dst), "v"(vh), "v"(vl), "n"(A_BYTES) : "memory");
                };
                unsigned char* dst = win_slot(0) + wv * 32 * CV_ROW + lane * 16;
                if (part & 1) pass(c_y[0], c_lb[0], dst);
                if (part & 2) {
                    pass(c_y[1], c_lb[1], dst + 16 * CV_ROW);
                    if (wv == 7 && lane < 8) pass(c_y[2], c_lb[2], win_slot(0) + CV_BM * CV_ROW + lane * 16);
                }
            };
            for (int i = tid; i < ZERO_BYTES / 4; i += NT) reinterpret_cast<uint32_t*>(smem + ZERO_BASE)[i] = 0u;
            const bool w0_src = nchw.c0 == 0;                // window 0 comes from src
            int c_ty = 0, c_p0 = 0;                           // tap row and first pixel of the fetch in flight
            if (w0_src) { c_p0 = fetch(0, 0); gw.advance(3); } else dma_a();
            dma_b(0);
            dma_b(1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                     // the zeroed area is every wave's to read
            if (w0_src) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * BP) : "memory");
                convert(0, c_p0, 3);
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BP) : "memory");
            } else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BP) : "memory");
            __builtin_amdgcn_s_barrier();
            if (grp == 1) __builtin_amdgcn_s_barrier();
            for (int g = 0; g < ngroups; ++g) {
                const bool lastg = g + 1 == ngroups;
                const bool nx = !lastg && gw.k0 >= nchw.c0;  // window g + 1 comes from src
                // ---- tx = 0 ----
                asm volatile("" ::: "memory");
                load_win();
                load_b(wt_slot(0), fbh, fbl);
                dma_b(2);                                     // stage 3g + 2
                if (nx) {
                    c_ty = gw.i; c_p0 = fetch(gw.i, gw.k0); gw.advance(3);
                    wait_barrier<BP + NP>();                  // stage 3g + 1 landed
                } else wait_barrier<BP>();
                mfmas(ah[0], al[0]);
                // ---- tx = 1 ----
                asm volatile("" ::: "memory");
                load_b(wt_slot(1), fbh, fbl);
                if (!lastg) {
                    dma_b(0);                                 // stage 3g + 3
                    if (nx) {                                 // the fetch (and stage 3g + 2, issued before it) landed
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BP) : "memory");
                        convert(c_ty, c_p0, 1);
                        wait_barrier<BP>();
                    } else {
                        dma_a();
                        if (wv == 0) wait_barrier<BP + AP + 2>(); else wait_barrier<BP + AP>();
                    }
                } else wait_barrier<0>();
                mfmas(ah[1], al[1]);
                // ---- tx = 2 ----
                asm volatile("" ::: "memory");
                load_b(wt_slot(2), fbh, fbl);
                if (!lastg) {
                    dma_b(1);                                 // stage 3g + 4
                    if (nx) convert(c_ty, c_p0, 2);
                    wait_barrier<BP>();                       // stage 3g + 3 landed, window g + 1 written
                } else wait_barrier<0>();
                mfmas(ah[2], al[2]);
            }
        } else {                                              // every other instance: the loop as it was (its lines left where they were)
        dma_a();
        dma_b(0);
        dma_b(1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BP) : "memory");                 // window 0 and stage 0 landed (this wave's pieces)
        __builtin_amdgcn_s_barrier();
        if (grp == 1) __builtin_amdgcn_s_barrier();           // group 1 runs one barrier (= half a sub-step) behind group 0
        for (int g = 0; g < ngroups; ++g) {
            const bool lastg = g + 1 == ngroups;
            // ---- tx = 0 ----
            asm volatile("" ::: "memory");
            load_win();
            load_b(wt_slot(0), fbh, fbl);
            dma_b(2);                                         // stage 3g + 2
            wait_barrier<BP>();                               // stage 3g + 1 landed
            mfmas(ah[0], al[0]);
            // ---- tx = 1 ----
            asm volatile("" ::: "memory");
            load_b(wt_slot(1), fbh, fbl);
            if (!lastg) {
                dma_b(0); dma_a();                            // stage 3g + 3, window g + 1
                if (wv == 0) wait_barrier<BP + AP + 2>(); else wait_barrier<BP + AP>();      // stage 3g + 2 landed
            } else wait_barrier<0>();
            mfmas(ah[1], al[1]);
            // ---- tx = 2 ----
            asm volatile("" ::: "memory");
            load_b(wt_slot(2), fbh, fbl);
            if (!lastg) { dma_b(1); wait_barrier<BP>(); }     // stage 3g + 4; stage 3g + 3 and window g + 1 landed
            else wait_barrier<0>();
            mfmas(ah[2], al[2]);
        }
        }
        if (grp == 0) __builtin_amdgcn_s_barrier();           // balance group 1's extra barrier
        __syncthreads();                                      // nothing in flight; the ring is dead
    } else
    if constexpr (WIN == 2) {
        // ---- row-window loop, prefetch distance 2 (3x3 layers): the window's fragments for all three tx live in REGISTERS
        // (read once per group), so one LDS window slot suffices and the weight tiles get a 3-slot ring: stage s+2's LDS-DMA is
        // issued right after the barrier of sub-step s and stays in flight across two barriers behind counted s_waitcnt vmcnt
        // (loads retire in order: "all but the pieces issued in the previous sub-step" = stage s landed).  Issuing the pieces
        // later in the sub-step, between the MFMAs, was measured 2.5 % slower, s_setprio around the MFMA block 1 % slower (same box A/B).  3 sub-steps per
        // group and 3 slots: stage s = 3g + tx lives in slot tx — every LDS address below is static.
        static_assert(!PP && SPB == 1 && NT == 256 && (BN % RP == 0 || BN == 32), "window loop with register-resident A: 4 waves, whole DMA passes (or the 32-wide case)");
        // Measured and rejected: the same loop with a 2-slot weight ring and a two-pass (2 x 64 rows) fused tail so that THREE
        // workgroups fit a CU (49 KB of LDS, <= 168 registers): 96 of the 168 registers hold the window, the compiler serialises the
        // weight fragment reads with the MFMAs: 9.4 vs 5.0 ms of convolutions per C2 step.
        // BN = 32 (F-Net's 32-wide trunk): the weight tile is 4 pieces of 16 rows — wave w stages plane w & 1, rows (w >> 1) * 16 ...,
        // ONE piece per wave, so the counted waits stay wave-uniform (row-pass staging would give waves 2 and 3 nothing to count)
        constexpr int BP = BN == 32 ? 1 : 2 * B_PT;           // weight-tile DMA instructions per wave and stage
        constexpr int AP = 2 * A_PT;                          // window DMA instructions per wave (wave 0: + 2 for the rows past the tile)
        const int aw = CV_BM + 2 * p.tap_sx;
        const int ngroups = 3 * ksteps_per_tap;               // (K chunk, ty) pairs, ty inner
        StepCounter gw, bs;                                   // next window (i = ty) / weight tile (i = tap) to fetch
        if constexpr (SPLITK) gw.k0 = bs.k0 = sk_c0 * CV_BK;  // the range's first channel: offset into the activation rows and the weight rows
        auto dma_a = [&]() { stage_window(win_slot(0), a_step(gw.i, 0, gw.k0), aw); gw.advance(3); };
        const int b_v32 = ((n0 + (wv >> 1) * 16 + (lane >> 2)) * p.cin + st_k) * 2;       // BN = 32: this wave's 16 weight rows
        auto dma_b = [&](int slot) {
            unsigned char* sb_hi = wt_slot(slot);
            const int b_u = (bs.i * p.cout_pad * p.cin + bs.k0) * 2;
            if constexpr (BN == 32) {
                if (wv & 1) CV_BLDS(rb_lo, sb_hi + B_BYTES + (wv >> 1) * 16 * CV_ROW, b_v32 + b_u);
                else        CV_BLDS(rb_hi, sb_hi + (wv >> 1) * 16 * CV_ROW, b_v32 + b_u);
            } else stage_weights(sb_hi, sb_hi + B_BYTES, b_u);
            bs.advance(9);
        };
        bf16x8_t ah[3][MF], al[3][MF];
        auto mfma_b = [&](int slot, const bf16x8_t (&xh)[MF], const bf16x8_t (&xl)[MF]) {
            bf16x8_t fbh[NFW], fbl[NFW];
            load_b(wt_slot(slot), fbh, fbl);
#pragma unroll
            for (int n = 0; n < NFW; ++n) mma3(n, xh, xl, fbh[n], fbl[n]);
        };
        dma_a();
        dma_b(0);
        dma_b(1);
        for (int g = 0; g < ngroups; ++g) {
            const bool lastg = g + 1 == ngroups;
            // ---- tx = 0: stage 3g (slot 0) and window g have landed; refill slot 2 with stage 3g + 2 ----
            wait_barrier<BP, true>();
            dma_b(2);
            // window g -> registers (spelled out here and a lambda in the 8-wave loop, as they were before the building blocks
            // were shared: in the other form either loop is scheduled differently)
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                for (int m = 0; m < MF; ++m) {
                    ah[tx][m] = ld_frag(win_slot(0) + a_offx[tx] + m * 16 * CV_ROW);
                    al[tx][m] = ld_frag(win_slot(0) + A_BYTES + a_offx[tx] + m * 16 * CV_ROW);
                }
            mfma_b(0, ah[0], al[0]);
            // ---- tx = 1: every wave holds window g in registers (lgkmcnt(0) before the barrier): fetch window g + 1 ----
            wait_barrier<BP, true>();
            if (!lastg) { dma_b(0); dma_a(); }
            mfma_b(1, ah[1], al[1]);
            // ---- tx = 2 (the window's pieces, issued after the weight pieces, stay in flight) ----
            if (!lastg) { wait_barrier<BP + AP, true>(); dma_b(1); }
            else wait_barrier<0, true>();
            mfma_b(2, ah[2], al[2]);
        }
        __syncthreads();                                      // nothing in flight; the ring is dead (the epilogue reuses it)
    } else if constexpr (WIN == 1) {
        static_assert(!PP && SPB == 1, "row-window loop: 2-slot ring");
        const int aw = CV_BM + (p.tap_n - 1) * p.tap_sx;      // window rows of this layer
        const int ngroups = p.tap_n * ksteps_per_tap;         // (K chunk, ty) pairs, ty inner
        StepCounter gw, bs;                                   // next window (i = ty) / weight tile (i = tap = ty*tap_n + tx) to fetch
        auto dma_a = [&](int slot) { stage_window(win_slot(slot), a_step(gw.i, 0, gw.k0), aw); gw.advance(p.tap_n); };
        auto dma_b = [&](int slot) { stage_weights(wt_slot(slot), wt_slot(slot) + B_BYTES, (bs.i * p.cout_pad * p.cin + bs.k0) * 2); bs.advance(p.taps); };
        dma_a(0);
        dma_b(0);
        __syncthreads();
        // ONE flat loop over the sub-steps (group g = (K chunk, ty), tx inner) with a single MFMA block per iteration: as a
        // g / tx loop nest the compiler peeled tx into three copies plus a remainder loop and resolved the accumulator phis
        // with 64 register moves (128 v_accvgpr moves before __launch_bounds__(NT, 2)) per group, draining the MFMA pipe.
        int bslot = 0, aslot = 0, tx = 0, a_of = a_offx[0];
        const int nsub = ngroups * p.tap_n;
        for (int s = 0; s < nsub; ++s) {
            const bool last_tx = tx + 1 == p.tap_n;
            if (s + 1 < nsub) dma_b(bslot ^ 1);                                    // next sub-step's weights
            if (last_tx && s + 1 < nsub) dma_a(aslot ^ 1);                         // next group's window
            compute(win_slot(aslot), wt_slot(bslot), a_of);
            __syncthreads();
            bslot ^= 1;
            if (last_tx) { tx = 0; aslot ^= 1; a_of = a_offx[0]; }
            else { ++tx; a_of = tx == 1 ? a_offx[1] : a_offx[2]; }
        }
    } else {
        // the 4-wave / 2-slot loop over (K chunk, tap) stages, no window: stage = A tile of tap (ty, tx) + its weight tile
        StepCounter pf;                                       // next stage to fetch: i = ty; with pf_tx, pf_tap = ty*tap_n + tx
        int pf_tx = 0, pf_tap = 0;
        if constexpr (SPLITK) pf.k0 = sk_c0 * CV_BK;
        auto dma = [&](int buf) {
            stage_window(win_slot(buf), a_step(pf.i, pf_tx, pf.k0), CV_BM);
            stage_weights(wt_slot(buf), wt_slot(buf) + B_BYTES, (pf_tap * p.cout_pad * p.cin + pf.k0) * 2);
            ++pf_tap;
            if (++pf_tx == p.tap_n) { pf_tx = 0; if (pf.advance(p.tap_n)) pf_tap = 0; }
        };
#pragma unroll
        for (int q = 0; q < SPB; ++q)
            if (q < nsteps) dma(q);
        __syncthreads();                                      // drains the DMA (vmcnt) and publishes the first half
        for (int s = 0, half = 0; s < nsteps; s += SPB, half ^= 1) {
            // the other half of the ring was last read one interval ago and every wave has passed that barrier:
            // refill it now, the DMA flies during this interval's MFMAs
#pragma unroll
            for (int q = 0; q < SPB; ++q)
                if (s + SPB + q < nsteps) dma((half ^ 1) * SPB + q);
#pragma unroll
            for (int q = 0; q < SPB; ++q)
                if (s + q < nsteps) {
                    if constexpr (F16) compute16(win_slot(half * SPB + q), wt_slot(half * SPB + q), a_off);
                    else compute(win_slot(half * SPB + q), wt_slot(half * SPB + q), a_off);
                }
            __syncthreads();                                  // next half landed; everyone done with this half
        }
    }
#undef CV_BLDS

    if constexpr (TAIL > 0) {
        // ---- fused 1x1 tail: the 128 x 128 tile (bias, ReLU, re-split) becomes the LDS-resident input of three 1x1 layers ----
        static_assert(NF == 8 && WN == 2 && ((CV_BM == 128 || CV_BM == 256) ? CV_BM == (NT / 64) * 32 : (CV_BM == 64 && NT == 256)),
                      "the fused tail is written for 128-channel tiles with 32 rows per wave (64-row tile: 4 waves of 32 rows x 64 channels)");
        unsigned char* act_hi = smem;                                   // [CV_BM rows][256 B]; the K ring is dead (barrier above)
        unsigned char* act_lo = smem + CV_BM * 256;
#pragma unroll
        for (int m = 0; m < MF; ++m)
#pragma unroll
            for (int n = 0; n < NFW; ++n) {                   // C^T accumulators (cv_mma<true>): 4 consecutive channels of one row
                const int trow = wm * (MF * 16) + m * 16 + (lane & 15);
                const int ch = wn * (NFW * 16) + n * 16 + (lane >> 4) * 4;
                float v[4] = {acc[m][n][0], acc[m][n][1], acc[m][n][2], acc[m][n][3]};   // includes ConvParams::addend (initial value)
                const float4 b4 = *reinterpret_cast<const float4*>(p.bias + ch);
                v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
                if (p.relu) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = v[r] < 0.f ? 0.f : v[r];
                }
                uint32_t h01, l01, h23, l23;
                split_bf16x2(v[0], v[1], h01, l01); split_bf16x2(v[2], v[3], h23, l23);
                const int off = act_swz(trow, ch >> 3) + (ch & 7) * 2;
                *reinterpret_cast<uint2*>(act_hi + off) = make_uint2(h01, h23);
                *reinterpret_cast<uint2*>(act_lo + off) = make_uint2(l01, l23);
            }
        __syncthreads();
        constexpr int NW = NT / 64;
        tail_layer_cols<8, false, CV_BM, NW>(p.tail_w_hi, p.tail_w_lo, p.tail_bias, act_hi, act_lo, nullptr, 0, row0, p.rows, lane, wv);
        tail_layer_cols<8, false, CV_BM, NW>(p.tail_w_hi + 128 * 128, p.tail_w_lo + 128 * 128, p.tail_bias + 128, act_hi, act_lo, nullptr,
                                             0, row0, p.rows, lane, wv);
        if constexpr (TAIL == 9) {
            if (p.up_out) {                           // fused convex upsampling: the 144 logits meet in LDS, never in HBM
                tail_layer_cols<9, true, CV_BM, NW, true, F16>(p.tail_w_hi + 2 * 128 * 128, p.tail_w_lo + 2 * 128 * 128, p.tail_bias + 256, act_hi,
                                                          act_lo, nullptr, 0, row0, p.rows, lane, wv,
                                                          UpArgs{p.up_depth, p.up_out, p.up_npred, p.up_h, p.up_w, p.up_B});
                return;
            }
        }
        tail_layer_cols<TAIL, true, CV_BM, NW>(p.tail_w_hi + 2 * 128 * 128, p.tail_w_lo + 2 * 128 * 128, p.tail_bias + 256, act_hi, act_lo,
                                               p.out_f32, p.tail_cout, row0, p.rows, lane, wv,
                                               (TAIL == 1 && p.gu_out) ? UpArgs{p.gu_in, p.gu_out, -1, p.up_h, p.up_w, p.up_B} : UpArgs{nullptr, nullptr, 0, 0, 0, 0});
        return;
    }

    if constexpr (SPLITK) {
        // ---- split-K: the raw accumulator tile -> sk_work[sk_z], through the plain epilogue's wave-private staging rows (16-byte stores
        // of 8 consecutive channels); rows < p.rows only, channels n0 .. n0 + BN - 1 < cout_pad (the grid's y extent) ----
        constexpr int WCOLS = NFW * 16, SROW = WCOLS + 4;
        float* stage = reinterpret_cast<float*>(smem) + wv * (16 * SROW);
        float* const wz = sk_work + (size_t)sk_z * (size_t)p.rows * p.cout_pad;
#pragma unroll
        for (int m = 0; m < MF; ++m) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int n = 0; n < NFW; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    stage[((lane >> 4) * 4 + r) * SROW + n * 16 + (lane & 15)] = acc[m][n][r];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int it = lane; it < 16 * (WCOLS / 8); it += 64) {
                const int r = it / (WCOLS / 8), c8 = (it % (WCOLS / 8)) * 8;
                const long long row = row0 + wm * (MF * 16) + m * 16 + r;
                if (row >= p.rows) continue;
                float* o = wz + (size_t)row * p.cout_pad + n0 + wn * WCOLS + c8;
                *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(stage + r * SROW + c8);
                *reinterpret_cast<float4*>(o + 4) = *reinterpret_cast<const float4*>(stage + r * SROW + c8 + 4);
            }
        }
        return;
    }

    // ---- epilogue through LDS, one 16-row fragment per wave at a time: [16 rows][NFW*16] fp32 per wave ----
    // Round 4 (profiles/r4/conv_no_epilogue.log): of the 8-wave kernel's 0.16 ms that do not depend on K (10 % of
    // the launch at K = 9 x 256), 0.13 ms is this epilogue = 6.6 us per tile = the tile's 128 KB at ~20 GB/s per CU — x 256 CUs in
    // lockstep (one workgroup per CU, equal tile times) 5 - 6 TB/s: the stores of all tiles arrive as ONE burst at the fabric's write
    // rate while the matrix pipes idle.  Tried against it: (1) persistent workgroups (profiles/r4/conv_persistent_ab.log; no gain: a wave's loads and
    // stores share vmcnt, so the next tile's first counted wait still drains the stores); (2) start skew of the first-round workgroups
    // by eighths of a tile time (conv_start_skew.log: fixed part 0.162 -> 0.118 ms, but the late starters end the launch late: +3 % at
    // K = 9 x 512, -2.6 % at K = 9 x 64, a wash at the G-Net shapes); (3) C^T accumulators stored straight from registers, no LDS stage
    // (conv_direct_epilogue.log: fp32 outputs -1.5 % at K = 9 x 128, but the bf16 planes leave as 8-byte stores = 32-byte row segments and
    // the F-Net slows down 18.4 -> 19.3 ms).  What would remove it is an epilogue that overlaps another tile's K loop on the same CU
    // (two co-resident workgroups out of phase: needs the 8-wave loop in <= 80 KB of LDS and <= 128 registers) — not built.
    const long long tile_img = p.img_rows ? row0 / p.img_rows : 0;            // wave-uniform (scalar) division, once
    const int tile_rem = p.img_rows ? (int)(row0 - tile_img * p.img_rows) : 0;
    const float inv_wp = 1.0f / (float)(p.wp > 0 ? p.wp : 1);
    constexpr int WCOLS = NFW * 16, SROW = WCOLS + 4;          // +4 floats row pad
    float* stage = reinterpret_cast<float*>(smem) + wv * (16 * SROW);
    // a lane's work items of every fragment cover the same 8 channels when 64 is a multiple of the items per row: its bias values are
    // loaded once per tile (they used to be re-loaded behind every staging read)
    constexpr bool BIAS_INV = (64 % (WCOLS / 8)) == 0;
    float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (BIAS_INV) {
        const int ch = n0 + wn * WCOLS + (lane % (WCOLS / 8)) * 8;
        const float4 b0 = *reinterpret_cast<const float4*>(p.bias + ch), b1 = *reinterpret_cast<const float4*>(p.bias + ch + 4);
        bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w; bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
    }
#pragma unroll
    // the staging rows are wave-private: after the K loop's final barrier (every wave is done with the ring) only the
    // wave's own LDS accesses need ordering — in-order in hardware, a scheduling fence for the compiler — no workgroup barrier
    for (int m = 0; m < MF; ++m) {                            // fully unrolled: acc indices stay static
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int n = 0; n < NFW; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                stage[((lane >> 4) * 4 + r) * SROW + n * 16 + (lane & 15)] = acc[m][n][r];   // C: col = lane&15, row = (lane>>4)*4+r
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // 16 rows x WCOLS channels, 8 channels (one 16-byte bf16 vector / two fp32 vectors) per work item
        for (int it = lane; it < 16 * (WCOLS / 8); it += 64) {
            const int r = it / (WCOLS / 8), c8 = (it % (WCOLS / 8)) * 8;
            const long long row = row0 + wm * (MF * 16) + m * 16 + r;
            if (row >= p.rows) continue;
            const int ch = n0 + wn * WCOLS + c8;
            long long orow = row;
            bool interior = true;
            if (p.img_rows) {                                 // row -> (image, y, x) of the zero-bordered grid
                // the tile's first row is decoded once per workgroup on the scalar unit (tile_img, tile_rem); per work item a
                // 32-bit add, a wrap and a float-reciprocal division by the row pitch (exact: img_rows < 2^24, fixed up)
                long long img = tile_img;
                int rem = tile_rem + (int)(row - row0);
                while (rem >= p.img_rows) { rem -= p.img_rows; ++img; }
                int y = (int)((float)rem * inv_wp);
                if (y * p.wp > rem) --y;
                if ((y + 1) * p.wp <= rem) ++y;
                const int x = rem - y * p.wp;
                interior = (y >= p.pad) && (y < p.hp - p.pad) && (x >= p.pad) && (x < p.wp - p.pad);
                if (p.repad) {
                    if (!interior) continue;
                    const int q = p.repad - 1, hh = p.hp - 2 * p.pad, ww = p.wp - 2 * p.pad;
                    orow = (img * (hh + 2 * q) + (y - p.pad + q)) * (ww + 2 * q) + (x - p.pad + q);
                }
            }
            float v[8];
            float ad[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if constexpr (F16P) {                             // residual input: ONE fp16 plane, 8 channels per 16-byte load
                if (p.add_hi) f16x8_unpack(*reinterpret_cast<const uint4*>(p.add_hi + (size_t)row * p.add_ld + ch), ad);
            } else
            if (p.add_hi) {                                   // residual input, stored as split bf16 planes
                const uint4 ah = *reinterpret_cast<const uint4*>(p.add_hi + (size_t)row * p.add_ld + ch);
                const uint4 al = *reinterpret_cast<const uint4*>(p.add_lo + (size_t)row * p.add_ld + ch);
                const uint32_t hw_[4] = {ah.x, ah.y, ah.z, ah.w}, lw_[4] = {al.x, al.y, al.z, al.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ad[2 * i]     = __uint_as_float(hw_[i] << 16) + __uint_as_float(lw_[i] << 16);
                    ad[2 * i + 1] = __uint_as_float(hw_[i] & 0xffff0000u) + __uint_as_float(lw_[i] & 0xffff0000u);
                }
            }
            if (p.addend) {                                   // loop-invariant partial sums computed once per forward
                const float4 a0 = *reinterpret_cast<const float4*>(p.addend + (size_t)row * p.addend_ld + ch);
                const float4 a1 = *reinterpret_cast<const float4*>(p.addend + (size_t)row * p.addend_ld + ch + 4);
                ad[0] = a0.x; ad[1] = a0.y; ad[2] = a0.z; ad[3] = a0.w; ad[4] = a1.x; ad[5] = a1.y; ad[6] = a1.z; ad[7] = a1.w;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float x = (stage[r * SROW + c8 + i] + ad[i]) + (BIAS_INV ? bv[i] : p.bias[ch + i]);
                v[i] = (x < 0.f) ? (p.relu ? 0.f : (p.leaky == 1 ? x * p.leaky_slope : x)) : x;
                if (!interior) v[i] = 0.f;
            }
            if (p.leaky == 2) {                               // SiLU (launch-uniform): silu(0) = 0 keeps the border rows zero
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = silu_f32(v[i]);
            }
            const size_t e = (size_t)orow * p.out_ld + ch;
            if constexpr (F16P) {
                if (p.out_mode == 3) {                        // one fp16 plane, saturating RNE (f16_bits_sat): the next layer's operand
                    *reinterpret_cast<uint4*>(p.out_hi + e) = f16x8_pack_sat(v);
                    continue;
                }
            }
            if (p.out_mode == 2) {                            // single bf16 plane (RNE): the matcher's bf16 feature storage
                uint32_t h[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) h[i] = f32x2_to_bf16x2_rne(v[2 * i], v[2 * i + 1]);
                *reinterpret_cast<uint4*>(p.out_hi + e) = make_uint4(h[0], h[1], h[2], h[3]);
            } else if (p.out_mode == 0) {
                uint32_t h[4], l[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) split_bf16x2(v[2 * i], v[2 * i + 1], h[i], l[i]);
                *reinterpret_cast<uint4*>(p.out_hi + e) = make_uint4(h[0], h[1], h[2], h[3]);
                *reinterpret_cast<uint4*>(p.out_lo + e) = make_uint4(l[0], l[1], l[2], l[3]);
            } else {
                *reinterpret_cast<float4*>(p.out_f32 + e) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(p.out_f32 + e + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
    }
#endif
}

template <int NF, int WN, int CV_BM, int SPB, int TAIL = 0, int NT = 256, bool PP = false, int WIN = 0>
__global__ __launch_bounds__(NT, 2) void conv_mfma_kernel(const ConvParams p) {
    conv_mfma_tile<NF, WN, CV_BM, SPB, TAIL, NT, PP, WIN>(p, blockIdx.x, gridDim.x, blockIdx.y, threadIdx.x);
}

// The fp32-source instances (magnet_conv_mfma_nchw): the 8-wave 256-row fused-tail loop with the NCHW flag, under a name of their own
template <int TAIL>
__global__ __launch_bounds__(512, 2) void conv_mfma_nchw_kernel(const ConvParams p, const ConvSrc src) {
    conv_mfma_tile<8, 2, 256, 1, TAIL, 512, true, 2, false, false, false, true>(p, blockIdx.x, gridDim.x, blockIdx.y, threadIdx.x, nullptr, 0, 1, src);
}

// The instances of the single-plane fp16 format: kernels of their own name, so the bf16x3 instances keep theirs
template <int NF, int WN, int CV_BM, int SPB, int TAIL, int NT, bool PP, int WIN>
__global__ __launch_bounds__(NT, 2) void conv_mfma_f16_kernel(const ConvParams p) {
    conv_mfma_tile<NF, WN, CV_BM, SPB, TAIL, NT, PP, WIN, true>(p, blockIdx.x, gridDim.x, blockIdx.y, threadIdx.x);
}

// The plane-to-plane instances (magnet_conv_mfma_f16p): again kernels of their own name
template <int NF, int WN, int CV_BM, int SPB, int TAIL, int NT, bool PP, int WIN>
__global__ __launch_bounds__(NT, 2) void conv_mfma_f16p_kernel(const ConvParams p) {
    conv_mfma_tile<NF, WN, CV_BM, SPB, TAIL, NT, PP, WIN, true, true>(p, blockIdx.x, gridDim.x, blockIdx.y, threadIdx.x);
}

// The split-K instances (magnet_conv_mfma_splitk): the 4-wave 128-row x 128-channel loops, WIN = 2 (3x3) and WIN = 0 (1x1); blockIdx.z =
// the split.  Kernels of their own name; the partials go to `work`, nothing else is written
template <int WIN>
__global__ __launch_bounds__(256, 2) void conv_mfma_splitk_kernel(const ConvParams p, float* __restrict__ work) {
    conv_mfma_tile<8, 2, 128, 1, 0, 256, false, WIN, false, false, true>(p, blockIdx.x, gridDim.x, blockIdx.y, threadIdx.x, work, blockIdx.z, gridDim.z);
}

// The D-Net decoder's wide fp16 instances (magnet_conv_mfma_f16d): plane to plane at 128 rows x 128 channels, blockIdx.y = the channel
// block; and their split-K form (magnet_conv_mfma_f16d_splitk).  Kernels of their own name again
template <int WIN>
__global__ __launch_bounds__(256, 2) void conv_mfma_f16d_kernel(const ConvParams p) {
    conv_mfma_tile<8, 2, 128, 1, 0, 256, false, WIN, true, true>(p, blockIdx.x, gridDim.x, blockIdx.y, threadIdx.x);
}
template <int WIN>
__global__ __launch_bounds__(256, 2) void conv_mfma_f16d_splitk_kernel(const ConvParams p, float* __restrict__ work) {
    conv_mfma_tile<8, 2, 128, 1, 0, 256, false, WIN, true, true, true>(p, blockIdx.x, gridDim.x, blockIdx.y, threadIdx.x, work, blockIdx.z, gridDim.z);
}

// out = epilogue(((p_0 + p_1) + p_2 ... ) + bias): the fixed-order fp32 sum of the S partials work[z][row][cout_pad], then what the plain
// epilogue applies — ReLU / LeakyReLU, zeros at border positions, repad re-addressing, out_ld channel slices — as split-bf16 planes
// (out_mode 0) or fp32 (out_mode 1); F16OUT (the reduce of magnet_conv_mfma_f16d_splitk): out_mode 3 (one fp16 plane at out_hi) besides.
// One thread = 8 channels of one row: 16-byte loads and stores, no LDS.
template <bool F16OUT>
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvParams p, const float* __restrict__ work, const int S) {
    const int c8n = p.cout_pad / 8;
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = it / c8n;
    if (row >= p.rows) return;
    const int ch = (int)(it - row * c8n) * 8;
    long long orow = row;
    bool interior = true;
    if (p.img_rows) {
        const long long img = row / p.img_rows;
        const int rem = (int)(row - img * p.img_rows), y = rem / p.wp, x = rem - y * p.wp;
        interior = (y >= p.pad) && (y < p.hp - p.pad) && (x >= p.pad) && (x < p.wp - p.pad);
        if (p.repad) {
            if (!interior) return;
            const int q = p.repad - 1, hh = p.hp - 2 * p.pad, ww = p.wp - 2 * p.pad;
            orow = (img * (hh + 2 * q) + (y - p.pad + q)) * (ww + 2 * q) + (x - p.pad + q);
        }
    }
    const size_t plane = (size_t)p.rows * p.cout_pad;
    const float* src = work + (size_t)row * p.cout_pad + ch;
    float4 q0[8], q1[8];                                      // every partial's loads are issued before the first addition
#pragma unroll
    for (int z = 0; z < 8; ++z)
        if (z < S) { q0[z] = *reinterpret_cast<const float4*>(src + z * plane); q1[z] = *reinterpret_cast<const float4*>(src + z * plane + 4); }
    float v[8] = {q0[0].x, q0[0].y, q0[0].z, q0[0].w, q1[0].x, q1[0].y, q1[0].z, q1[0].w};
#pragma unroll
    for (int z = 1; z < 8; ++z)
        if (z < S) {
            v[0] += q0[z].x; v[1] += q0[z].y; v[2] += q0[z].z; v[3] += q0[z].w;
            v[4] += q1[z].x; v[5] += q1[z].y; v[6] += q1[z].z; v[7] += q1[z].w;
        }
    const float4 b0 = *reinterpret_cast<const float4*>(p.bias + ch), b1 = *reinterpret_cast<const float4*>(p.bias + ch + 4);
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = v[i] + bv[i];
        v[i] = (x < 0.f) ? (p.relu ? 0.f : (p.leaky ? x * p.leaky_slope : x)) : x;
        if (!interior) v[i] = 0.f;
    }
    const size_t e = (size_t)orow * p.out_ld + ch;
    if constexpr (F16OUT) {
        if (p.out_mode == 3) {                                // one fp16 plane, saturating RNE (f16_bits_sat), as the plain epilogue's
            *reinterpret_cast<uint4*>(p.out_hi + e) = f16x8_pack_sat(v);
            return;
        }
    }
    if (p.out_mode == 0) {
        uint32_t h[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split_bf16x2(v[2 * i], v[2 * i + 1], h[i], l[i]);
        *reinterpret_cast<uint4*>(p.out_hi + e) = make_uint4(h[0], h[1], h[2], h[3]);
        *reinterpret_cast<uint4*>(p.out_lo + e) = make_uint4(l[0], l[1], l[2], l[3]);
    } else {
        *reinterpret_cast<float4*>(p.out_f32 + e) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p.out_f32 + e + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
}

template <int NF, int WN, int BM, int SPB, int NT = 256, bool PP = false, int WIN = 0, bool F16 = false>
constexpr size_t conv_lds_bytes_c = ConvLds<NF, WN, BM, SPB, NT, PP, WIN, F16>::TOTAL;
template <int NF, int WN, int BM, int SPB, int NT = 256, bool PP = false, int WIN = 0, bool F16 = false>
static size_t conv_lds_bytes() { return ConvLds<NF, WN, BM, SPB, NT, PP, WIN, F16>::TOTAL; }

// > 64 KiB of dynamic LDS needs the opt-in attribute: set once per kernel and process (`done`: the launching instance's static flag)
static void lds_opt_in(const void* kernel, size_t lds, bool& done) {
    if (!done && lds > 64 * 1024) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        done = true;
    }
}

template <int NF, int WN, int BM, int SPB, int TAIL = 0, int NT = 256, bool PP = false, int WIN = 0, bool F16 = false, bool F16P = false>
static hipError_t launch_conv_nf(const ConvParams& p_in, hipStream_t s) {
    // row tiles: the launches with a fused Gaussian update / upsampling know their image geometry (up_B, up_h, wp; rows checked by the
    // API) and write interior positions only, so each image can be tiled on its own without its top and bottom border image rows —
    // taken when that is fewer tiles (conv_row_tiles; 64 frames of 120x160: 4 864 = 19 x 256 instead of 4 941).  MAGNET_TILING_FLAT
    // (MagnetConvExArgs; dev library: MAGNET_CONV_VARIANT bit 4096) keeps the flat form: same kernel, the other row0 formula.
    ConvParams p = p_in;
    long long n_tiles = (p.rows + BM - 1) / BM;
    p.tiles_per_img = 0;
    if (p.up_B > 0 && (p.gu_out || p.up_out) && !(p.tiling & 1) && !(p.variant & 4096))
        n_tiles = conv_row_tiles(p.up_B, p.up_h, p.wp, BM, &p.tiles_per_img);
    if (p.tiles_out) *p.tiles_out = n_tiles;
    dim3 grid((unsigned)n_tiles, (unsigned)(p.cout_pad / (NF * 16))), block(NT);
    size_t lds = conv_lds_bytes<NF, WN, BM, SPB, NT, PP, WIN, F16>();
    if (TAIL > 0 && lds < (size_t)BM * 512) lds = (size_t)BM * 512;     // the fused tail's activation tile: BM rows x 256 B x (hi, lo)
    constexpr size_t UP_STAGE = (size_t)(BM < 128 ? BM : 128) * 148 * 4;   // fused upsampling (tail_layer_cols: HR rows x SP floats): 128 (or BM = 64) rows x 144 logits (+4 pad) fp32
    if (TAIL == 9 && lds < UP_STAGE) lds = UP_STAGE;                        // (two 4-wave workgroups still fit a CU)
    void (*const kernel)(const ConvParams) = [] {
        if constexpr (F16P) return &conv_mfma_f16p_kernel<NF, WN, BM, SPB, TAIL, NT, PP, WIN>;
        else if constexpr (F16) return &conv_mfma_f16_kernel<NF, WN, BM, SPB, TAIL, NT, PP, WIN>;
        else return &conv_mfma_kernel<NF, WN, BM, SPB, TAIL, NT, PP, WIN>;
    }();
    static bool attr_set = false;
    lds_opt_in(reinterpret_cast<const void*>(kernel), lds, attr_set);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, p);
    return hipGetLastError();
}

// The fused-tail instance of one K loop <BM, NT, PP, WIN> for the tail's last layer: 16 (G-Net head), 128 or 144 (mask head) channels
template <int BM, int NT, bool PP, int WIN>
static hipError_t launch_conv_tail(const ConvParams& p, hipStream_t s) {
    switch (p.tail_cout) {
    case 16:  return launch_conv_nf<8, 2, BM, 1, 1, NT, PP, WIN>(p, s);
    case 128: return launch_conv_nf<8, 2, BM, 1, 8, NT, PP, WIN>(p, s);
    case 144: return launch_conv_nf<8, 2, BM, 1, 9, NT, PP, WIN>(p, s);
    default:  return hipErrorInvalidValue;
    }
}

// The fp32-source form (magnet_conv_mfma_nchw, which has checked what it serves): the 256-row 8-wave loop with the fused tail of G-Net
// (Gaussian update) or the mask head (upsampling), per-image tiling in effect.  The LDS request is launch_conv_nf's for these tails,
// BM * 512 bytes: the staging area lives behind the ring inside it (conv_mfma_tile asserts that it fits)
template <int TAIL>
static hipError_t launch_conv_nchw_tail(const ConvParams& p_in, const ConvSrc& src, hipStream_t s) {
    ConvParams p = p_in;
    const long long n_tiles = conv_row_tiles(p.up_B, p.up_h, p.wp, 256, &p.tiles_per_img);
    if (!p.tiles_per_img) return hipErrorInvalidValue;             // a tile must lie inside ONE image
    if (p.tiles_out) *p.tiles_out = n_tiles;
    constexpr size_t lds = 256 * 512;
    static_assert(lds >= conv_lds_bytes_c<8, 2, 256, 1, 512, true, 2>, "the ring fits the fused tail's request");
    static bool attr_set = false;
    lds_opt_in(reinterpret_cast<const void*>(&conv_mfma_nchw_kernel<TAIL>), lds, attr_set);
    hipLaunchKernelGGL(conv_mfma_nchw_kernel<TAIL>, dim3((unsigned)n_tiles, 1), dim3(512), lds, s, p, src);
    return hipGetLastError();
}

static hipError_t launch_conv_nchw(const ConvParams& p, const ConvSrc& src, hipStream_t s) {
    if (!src.ptr || !p.tail_w_hi || p.cout_pad != 128 || p.tap_n != 3 || p.tap_sx != 1 || p.addend || p.variant || (p.tiling & ~2) ||
        !(p.rows >= 256ll * 256 || (p.tiling & 2)) || p.up_B <= 0 || src.c0 < 0 || src.c0 >= p.cin)
        return hipErrorInvalidValue;
    if (p.tail_cout == 16 && p.gu_out) return launch_conv_nchw_tail<1>(p, src, s);
    if (p.tail_cout == 144 && p.up_out) return launch_conv_nchw_tail<9>(p, src, s);
    return hipErrorInvalidValue;
}

// The (hi, lo) plane format (CONV_BF16X3; magnet_conv_mfma and magnet_conv_mfma_ex)
static hipError_t launch_conv_mfma(const ConvParams& p, hipStream_t s) {
    // p.variant is 0 in the product library; the dev library takes it from MAGNET_CONV_VARIANT.  Each bit only moves a launch to an
    // instance that other shapes reach anyway: 1 = no row window, 8 = the 2-slot LDS window instead of the register window, 16 = the
    // 4-wave register-window loop where the 8-wave one is the default, 256 / 2048 = the 8-wave loop for addend / split-bf16 launches,
    // 4096 = flat row tiling where per-image tiling is the default (launch_conv_nf).
    // 128 channels: 2x2 waves of 64x64 on a 128-row tile.
    // Measured alternatives on the G-Net 3x3 layer (64 frames; this configuration: 2.31 ms): 64-row tile / 3 workgroups
    // per CU 2.80 ms; two K stages per barrier (4-stage ring, 128 KB LDS, 1 workgroup per CU) 3.51 ms; 256-row tile
    // (1 workgroup per CU) 3.45 ms.  The kernel lives on inter-workgroup overlap: keep 2 workgroups per CU.
    if (p.tail_w_hi) {                           // 3x3 (or 1x1) 128-wide layer + its three 1x1 successors in one kernel
        if (p.cout_pad != 128) return hipErrorInvalidValue;
        const bool win = p.tap_n > 1 && !(p.variant & 1);
        // MAGNET_TILING_BM64 (latency mode): 64-row tiles of the 4-wave register-window loop.  One frame of 120x160 is 152 tiles of 128
        // rows for 256 CUs; as 304 tiles of 64 rows every CU has work and part of the chip holds the two workgroups this loop is
        // built around.  Same K order per output element and the same per-row tail arithmetic: bit-identical to the other tile sizes.
        // The caller asks for it (ConvStackMFMA.small_tiles decides by tile count); the API has checked that this instance exists.
        if (p.tiling & 4) return p.tap_n == 3 ? launch_conv_tail<64, 256, false, 2>(p, s) : hipErrorInvalidValue;
        // default: ping-pong x register window, 256-row tile, 8 waves — when there is at least one such tile per CU (256 CUs);
        // fewer rows (single-frame inference: 78 tiles at 120x160) spread better as 128-row tiles of the 4-wave kernel
        // — and not for the per-iteration launches of a hoisted first layer (fp32 addend, K = 9 x 32 .. 9 x 64): those are short K
        // loops between an exposed 128 KB addend load and the tail, where two co-resident 4-wave workgroups overlap better than one
        // 8-wave workgroup (same-box A/B: 425 vs 464 us at K = 288, 766 vs 804 us at K = 576)
        // (MAGNET_TILING_BM256 of MagnetConvExArgs takes it at any row count: the tests reach its tile edges with small grids)
        if (win && p.tap_n == 3 && !(p.variant & (16 | 8)) && (p.rows >= 256ll * 256 || (p.tiling & 2)) && (!p.addend || (p.variant & 256)))
            return launch_conv_tail<256, 512, true, 2>(p, s);
        if (win && p.tap_n == 3 && !(p.variant & 8)) return launch_conv_tail<128, 256, false, 2>(p, s);
        if (win) return launch_conv_tail<128, 256, false, 1>(p, s);
        return launch_conv_tail<128, 256, false, 0>(p, s);
    }
    // the loop-invariant x_d3 part of G-Net's first layer (fp32 partial sums, I >= 2): the fused-tail kernels' 8-wave ping-pong x
    // register-window loop (same-box: C3 step -1 %); on the F-Net's plain 128-wide layers (split-bf16 outputs) it is equal to the
    // 4-wave loop (18.64 - 18.72 vs 18.69 - 18.75 ms per 40 images; dev MAGNET_CONV_VARIANT=2048 forces it there)
    if (p.tiling & 4)                           // MAGNET_TILING_BM64: the plain 128-wide 3x3 layer on 64-row tiles (every output mode)
        return (p.cout_pad % 128 == 0 && p.tap_n == 3) ? launch_conv_nf<8, 2, 64, 1, 0, 256, false, 2>(p, s) : hipErrorInvalidValue;
    if (p.cout_pad == 128 && p.tap_n == 3 && (p.out_mode == 1 || (p.variant & 2048)) && !(p.variant & (16 | 9)) && p.rows >= 256ll * 256 && !p.add_hi && !p.img_rows)
        return launch_conv_nf<8, 2, 256, 1, 0, 512, true, 2>(p, s);
    if (p.cout_pad % 128 == 0 && p.tap_n == 3 && !(p.variant & 9)) return launch_conv_nf<8, 2, 128, 1, 0, 256, false, 2>(p, s);
    if (p.cout_pad % 128 == 0 && p.tap_n > 1 && !(p.variant & 1)) return launch_conv_nf<8, 2, 128, 1, 0, 256, false, 1>(p, s);
    if (p.cout_pad % 128 == 0) return launch_conv_nf<8, 2, 128, 1>(p, s);
    if (p.cout_pad == 144) return launch_conv_nf<9, 1, 128, 1>(p, s);
    if (p.cout_pad == 16)  return launch_conv_nf<1, 1, 128, 1>(p, s);
    // F-Net trunk widths: 4 waves stacked along M.  Measured on the whole F-Net (40 images, 23.5 ms): 256-row tiles for
    // the 32- / 64-wide layers 24.1 / 24.2 ms, 192-row tile for 64-wide 24.6 ms, 2x2 waves for 64-wide 23.6 ms — no better.
    // 32- and 64-wide 3x3 layers of the trunk: the register-window loop too (their A operand is 2/3 of the DMA pieces of a K step)
    // (round 3, with the register window: 256-row tiles = 64 rows per wave for the 64-wide layers 18.5 vs 18.0 ms per 40 images, for the
    // 32-wide ones 18.1 vs 18.0 — their fragment-read share was not the limit; not kept)
    if (p.cout_pad == 32 && p.tap_n == 3 && !(p.variant & 9))  return launch_conv_nf<2, 1, 128, 1, 0, 256, false, 2>(p, s);
    if (p.cout_pad == 64 && p.tap_n == 3 && !(p.variant & 9))  return launch_conv_nf<4, 1, 128, 1, 0, 256, false, 2>(p, s);
    if (p.cout_pad == 32)  return launch_conv_nf<2, 1, 128, 1>(p, s);
    if (p.cout_pad == 64)  return launch_conv_nf<4, 1, 128, 1>(p, s);
    return hipErrorInvalidValue;
}

// The single-plane fp16 format (magnet_conv_mfma_f16): the launches MAGNET._refine_mfma makes and nothing else — the 3x3 layer with
// the fused tail of G-Net (16 outputs) or the mask head (144), and the plain 128-wide 3x3 layer with fp32 output (the loop-invariant
// part of G-Net's first layer).  The API has refused every other form.  Tile selection is launch_conv_mfma's: 256-row 8-wave tiles from
// 65 536 rows on (or under MAGNET_TILING_BM256), except for the short per-iteration launches that carry an addend.
static hipError_t launch_conv_mfma_f16(const ConvParams& p, hipStream_t s) {
    const bool big = p.rows >= 256ll * 256 || (p.tiling & 2);
    if (p.tail_w_hi) {
        if (big && !p.addend) {
            if (p.tail_cout == 16) return launch_conv_nf<8, 2, 256, 1, 1, 512, true, 2, true>(p, s);
            if (p.tail_cout == 144) return launch_conv_nf<8, 2, 256, 1, 9, 512, true, 2, true>(p, s);
            return hipErrorInvalidValue;
        }
        if (p.tail_cout == 16) return launch_conv_nf<8, 2, 128, 1, 1, 256, false, 2, true>(p, s);
        if (p.tail_cout == 144) return launch_conv_nf<8, 2, 128, 1, 9, 256, false, 2, true>(p, s);
        return hipErrorInvalidValue;
    }
    if (big) return launch_conv_nf<8, 2, 256, 1, 0, 512, true, 2, true>(p, s);
    return launch_conv_nf<8, 2, 128, 1, 0, 256, false, 2, true>(p, s);
}

// The single-plane fp16 format, plane to plane (magnet_conv_mfma_f16p): the F-Net's launches — taps 9 (any dilation), 4 and 1 at 32,
// 64 and 128 output channels, fp16 residual plane, fp16 / fp32 / single-bf16 output, channel slices, zero border, repad.  The API has
// refused the fused tail, the addend and the BM64 / BM256 tilings.  Tiles are chosen as launch_conv_mfma chooses them
// for the F-Net's launches (which carry img_rows, a residual or a 2-byte output: never the 256-row form): 128 rows, 4 waves; 3x3 on the
// register-window loop, 1x1 and 2x2 windows on the windowless loop.
static hipError_t launch_conv_mfma_f16p(const ConvParams& p, hipStream_t s) {
    if (p.tap_n == 3) {
        if (p.cout_pad == 128) return launch_conv_nf<8, 2, 128, 1, 0, 256, false, 2, true, true>(p, s);
        if (p.cout_pad == 64)  return launch_conv_nf<4, 1, 128, 1, 0, 256, false, 2, true, true>(p, s);
        if (p.cout_pad == 32)  return launch_conv_nf<2, 1, 128, 1, 0, 256, false, 2, true, true>(p, s);
        return hipErrorInvalidValue;
    }
    if (p.cout_pad == 128) return launch_conv_nf<8, 2, 128, 1, 0, 256, false, 0, true, true>(p, s);
    if (p.cout_pad == 64)  return launch_conv_nf<4, 1, 128, 1, 0, 256, false, 0, true, true>(p, s);
    if (p.cout_pad == 32)  return launch_conv_nf<2, 1, 128, 1, 0, 256, false, 0, true, true>(p, s);
    return hipErrorInvalidValue;
}

// The fixed tile <8, 2, 128, 1, 0, 256, false, WIN> on the (row tiles, cout_pad / 128[, S]) grid, flat tiling.  S == 0: the plain launch
// of the D-Net decoder's wide fp16 layers.  S >= 2: the split-K partials of either operand format, S launches in one grid (z = the
// split) into `work` (S x rows x cout_pad fp32); the (hi, lo) format has no plain launch here (launch_conv_mfma serves it)
template <bool F16, int WIN>
static hipError_t launch_wide(const ConvParams& p_in, int S, float* work, hipStream_t s) {
    if (!F16 && !S) return hipErrorInvalidValue;                   // no plain (hi, lo) instance here; launch_conv never asks for one
    ConvParams p = p_in;
    p.tiles_per_img = 0;
    if (p.tiles_out) *p.tiles_out = (p.rows + 127) / 128;
    const size_t lds = conv_lds_bytes<8, 2, 128, 1, 256, false, WIN, F16>();     // fp16: 33 280 / 32 768 bytes, no opt-in attribute
    static_assert(!F16 || ConvLds<8, 2, 128, 1, 256, false, WIN, true>::TOTAL <= 64 * 1024, "dynamic LDS within the default limit");
    const dim3 grid((unsigned)((p.rows + 127) / 128), (unsigned)(p.cout_pad / 128), (unsigned)(S ? S : 1));
    if constexpr (F16) {
        if (!S) {                                                  // the plain launch
            hipLaunchKernelGGL(conv_mfma_f16d_kernel<WIN>, grid, dim3(256), lds, s, p);
            return hipGetLastError();
        }
    }
    void (*const kernel)(const ConvParams, float*) = [] {
        if constexpr (F16) return &conv_mfma_f16d_splitk_kernel<WIN>;
        else return &conv_mfma_splitk_kernel<WIN>;
    }();
    static bool attr_set = false;
    lds_opt_in(reinterpret_cast<const void*>(kernel), lds, attr_set);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, p, work);
    return hipGetLastError();
}

// Split-K (magnet_conv_mfma_splitk, magnet_conv_mfma_f16d_splitk; the API has checked the form): the partials, then the reduce launch
// on the same stream.  No counters, no atomics: two ordinary launches.
template <bool F16>
static hipError_t launch_splitk(const ConvParams& p, int S, float* work, hipStream_t s) {
    const hipError_t e = p.tap_n == 3 ? launch_wide<F16, 2>(p, S, work, s) : launch_wide<F16, 0>(p, S, work, s);
    if (e != hipSuccess) return e;
    const long long items = p.rows * (p.cout_pad / 8);
    hipLaunchKernelGGL(conv_splitk_reduce_kernel<F16>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p, work, S);
    return hipGetLastError();
}

// The D-Net decoder's plain layers on fp16 planes (magnet_conv_mfma_f16d): taps 9 / 1, any cout_pad % 128 == 0 (blockIdx.y = the channel
// block), LeakyReLU, fp16 / fp32 / split-bf16 output.  The API has refused everything else.  128-row tiles, 4 waves, flat tiling.
static hipError_t launch_conv_mfma_f16d(const ConvParams& p, hipStream_t s) {
    return p.tap_n == 3 ? launch_wide<true, 2>(p, 0, nullptr, s) : launch_wide<true, 0>(p, 0, nullptr, s);
}

// The EfficientNet encoder's 1x1 layers on fp16 planes (magnet_conv_mfma_f16e): SiLU or none, an optional fp16 residual plane, fp16 /
// fp32 output.  No instance of its own: 32 and 64 outputs run the windowless plane-to-plane instances of launch_conv_mfma_f16p, any
// cout_pad % 128 == 0 the wide instance of launch_conv_mfma_f16d (whose plain epilogue reads the residual and applies SiLU already)
static hipError_t launch_conv_mfma_f16e(const ConvParams& p, hipStream_t s) {
    if (p.cout_pad == 64)  return launch_conv_nf<4, 1, 128, 1, 0, 256, false, 0, true, true>(p, s);
    if (p.cout_pad == 32)  return launch_conv_nf<2, 1, 128, 1, 0, 256, false, 0, true, true>(p, s);
    return launch_wide<true, 0>(p, 0, nullptr, s);
}

// What each route's instances serve, as the API has checked it before: the launchers' own refusal of anything else
static bool route_serves(const ConvParams& p, ConvRoute route, int S, const float* work) {
    if (S && (S < 2 || S > 8 || !work)) return false;
    const bool plain = !(p.tail_w_hi || p.addend || (p.tiling & ~1));
    const bool wide = p.cout_pad % 128 == 0 && (p.tap_n == 3 || p.tap_n == 1);           // the shapes of launch_wide
    switch (route) {
    case CONV_BF16X3: return !S || wide;                           // S == 0: launch_conv_mfma refuses what has no instance
    case CONV_F16:    return !S && p.cout_pad == 128 && p.tap_n == 3;
    case CONV_F16P:   return !S && plain;
    case CONV_F16D:   return plain && !p.add_hi && wide;
    case CONV_F16E:   return !S && plain && p.tap_n == 1 && (p.cout_pad == 32 || p.cout_pad == 64 || wide);
    }
    return false;
}

hipError_t launch_conv(const ConvParams& p, ConvRoute route, int S, float* work, hipStream_t s, const ConvSrc* nchw) {
    if (!route_serves(p, route, S, work)) return hipErrorInvalidValue;
    if (nchw) return (route == CONV_BF16X3 && !S) ? launch_conv_nchw(p, *nchw, s) : hipErrorInvalidValue;
    switch (route) {
    case CONV_BF16X3: return S ? launch_splitk<false>(p, S, work, s) : launch_conv_mfma(p, s);
    case CONV_F16:    return S ? hipErrorInvalidValue : launch_conv_mfma_f16(p, s);
    case CONV_F16P:   return S ? hipErrorInvalidValue : launch_conv_mfma_f16p(p, s);
    case CONV_F16D:   return S ? launch_splitk<true>(p, S, work, s) : launch_conv_mfma_f16d(p, s);
    case CONV_F16E:   return S ? hipErrorInvalidValue : launch_conv_mfma_f16e(p, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace magnet
