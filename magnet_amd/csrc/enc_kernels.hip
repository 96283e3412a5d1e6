// enc_kernels.hip — the layers of the D-Net's EfficientNet-B5 encoder (magnet_amd/encoder.py; reference
// models/submodules/D_dense_depth.py:7-25) that are not matrix-core convolutions:
//   stem       3 -> 48 channels, 3x3 stride 2 with TF "SAME" padding (+ folded BatchNorm, SiLU), reads the NCHW fp32 image
//   dwconv     depthwise k x k (k 3 / 5, stride 1 / 2, explicit top / left padding) + folded BatchNorm + SiLU, and per-workgroup
//              partial channel sums of its outputs for the squeeze
//   se_gate    partial sums -> mean -> reduce FC, SiLU, expand FC, sigmoid: one gate per (image, channel)
//   se_scale   planes <- split((hi + lo) * gate)
// Activations are the conv kernel's format: zero-bordered channel-last grids (N, h+2, w+2, C_pad) stored as two bf16 planes
// (hi = bf16(x), lo = bf16(x - hi)), C_pad a multiple of 32, pad channels and border rows zero.  All are HBM-bound kernels with
// 16-byte accesses, 8 channels per thread.  No atomics anywhere: every output element has exactly one writer.
// The stem, the depthwise convolution and the scale are templates on the storage format: F16 = ONE fp16 plane per grid (the `_f16` entry
// points, EncoderMFMA(precision="fp16")): the same geometry, arithmetic and order; a load is one 16-byte access (f16x8_unpack, exact), a
// store is f16x8_pack_sat (saturating round-to-nearest-even), and the lo pointers are NULL and never touched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "enc_common.hpp"

namespace magnet {

namespace {

__device__ __forceinline__ uint16_t ek_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
template <bool F16>
__device__ __forceinline__ void ek_store8(uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, const size_t e, const float* v) {
    if constexpr (F16) {
        *reinterpret_cast<uint4*>(hi + e) = f16x8_pack_sat(v);
        return;
    }
    uint32_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint16_t h0 = ek_bf16(v[2 * i]), h1 = ek_bf16(v[2 * i + 1]);
        const uint16_t l0 = ek_bf16(v[2 * i] - __uint_as_float((uint32_t)h0 << 16));
        const uint16_t l1 = ek_bf16(v[2 * i + 1] - __uint_as_float((uint32_t)h1 << 16));
        h[i] = (uint32_t)h0 | ((uint32_t)h1 << 16);
        l[i] = (uint32_t)l0 | ((uint32_t)l1 << 16);
    }
    *reinterpret_cast<uint4*>(hi + e) = make_uint4(h[0], h[1], h[2], h[3]);
    *reinterpret_cast<uint4*>(lo + e) = make_uint4(l[0], l[1], l[2], l[3]);
}
template <bool F16>
__device__ __forceinline__ void ek_load8(const uint16_t* __restrict__ hi, const uint16_t* __restrict__ lo, const size_t e, float* v) {
    if constexpr (F16) {
        f16x8_unpack(*reinterpret_cast<const uint4*>(hi + e), v);
        return;
    }
    const uint4 a = *reinterpret_cast<const uint4*>(hi + e), b = *reinterpret_cast<const uint4*>(lo + e);
    const uint32_t h[4] = {a.x, a.y, a.z, a.w}, l[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i]     = __uint_as_float(h[i] << 16) + __uint_as_float(l[i] << 16);
        v[2 * i + 1] = __uint_as_float(h[i] & 0xffff0000u) + __uint_as_float(l[i] & 0xffff0000u);
    }
}

template <bool F16>
__device__ __forceinline__ void ek_zero8(uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, const size_t e) {
    const uint4 z = make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4*>(hi + e) = z;
    if constexpr (!F16) *reinterpret_cast<uint4*>(lo + e) = z;
}

}  // namespace

// ---- stem: out[n, y, x, co] = silu(b[co] + sum_{ci,dy,dx} W[co][ci][dy][dx] * img[n, ci, 2y+dy-pt, 2x+dx-pl]) ----
// one thread per output pixel; the 1 296 weights are read with wave-uniform addresses (scalar loads).  Channels 48..63 are written zero.
template <bool F16>
__global__ __launch_bounds__(256) void enc_stem_kernel(const float* __restrict__ img, const float* __restrict__ wgt,
                                                       const float* __restrict__ bias, uint16_t* __restrict__ out_hi,
                                                       uint16_t* __restrict__ out_lo, int N, int H, int W, int H2, int W2, int pt, int pl) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * H2 * W2) return;
    const int x = (int)(idx % W2), y = (int)((idx / W2) % H2), n = (int)(idx / ((long long)W2 * H2));
    float in[27];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = 2 * y + dy - pt, ix = 2 * x + dx - pl;
                const bool ok = (iy >= 0) && (iy < H) && (ix >= 0) && (ix < W);
                in[ci * 9 + dy * 3 + dx] = ok ? img[(((size_t)n * 3 + ci) * H + iy) * W + ix] : 0.f;
            }
    const size_t row = ((size_t)n * (H2 + 2) + (y + 1)) * (W2 + 2) + (x + 1);
#pragma unroll
    for (int c8 = 0; c8 < 6; ++c8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int co = c8 * 8 + i;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 27; ++k) acc = __builtin_fmaf(wgt[co * 27 + k], in[k], acc);
            v[i] = silu_f32(acc + bias[co]);
        }
        ek_store8<F16>(out_hi, out_lo, row * 64 + c8 * 8, v);
    }
#pragma unroll
    for (int c8 = 6; c8 < 8; ++c8) ek_zero8<F16>(out_hi, out_lo, row * 64 + c8 * 8);
}

// out_lo == NULL: out_hi is ONE fp16 plane (magnet_enc_stem_f16)
hipError_t launch_enc_stem(const float* img, const float* wgt, const float* bias, uint16_t* out_hi, uint16_t* out_lo, int N, int H, int W,
                           bool f16, hipStream_t s) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    const int th = (H2 - 1) * 2 + 3 - H, tw = (W2 - 1) * 2 + 3 - W;          // total TF-SAME padding (>= 0 for k 3, stride 2)
    const long long n = (long long)N * H2 * W2;
    const dim3 grid((unsigned)((n + 255) / 256));
    const int pt = (th > 0 ? th : 0) / 2, pl = (tw > 0 ? tw : 0) / 2;
    if (f16) hipLaunchKernelGGL(enc_stem_kernel<true>, grid, dim3(256), 0, s, img, wgt, bias, out_hi, nullptr, N, H, W, H2, W2, pt, pl);
    else hipLaunchKernelGGL(enc_stem_kernel<false>, grid, dim3(256), 0, s, img, wgt, bias, out_hi, out_lo, N, H, W, H2, W2, pt, pl);
    return hipGetLastError();
}

// ---- depthwise convolution ----
// A workgroup owns one image, one ENC_DW_TH x ENC_DW_TW tile of output pixels and CGB (4 or 8) groups of 8 channels; blockDim = 32 * CGB.
// A thread owns one 8-channel group and a strip of 4 consecutive output pixels of one row: for each of the K window rows it walks
// the (3 S + K) input pixels the strip touches ONCE (16 bytes of each plane), and every pixel feeds all the outputs whose window
// holds it from registers — K (3 S + K) / 4 pixel loads per output instead of K K.  Out-of-image taps are decided by index and
// skipped (the accumulator is untouched), so a 5x5 window never needs a 2-wide border.  Accumulation order per output: ky ascending,
// then kx ascending, fp32 fmaf.
// The partial sums: each thread adds its (up to 4) in-image outputs in x order, the workgroup adds the 32 strips in strip order
// through LDS, and thread (group, lane) of the first strip row writes part[n][tile][channels]: one writer, written exactly once.
template <int K, int S, bool F16>
__global__ __launch_bounds__(256) void enc_dwconv_kernel(const EncDwParams p) {
    extern __shared__ float red[];                            // [32 strips][CGB * 8]
    const int cgb = blockDim.x >> 5;
    const int g = threadIdx.x % cgb, strip = threadIdx.x / cgb;             // strip 0..31: 4 across, 8 down
    const int tiles_x = (p.wo + ENC_DW_TW - 1) / ENC_DW_TW;
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int n = blockIdx.z;
    const int c = (blockIdx.y * cgb + g) * 8;
    const int oy = ty * ENC_DW_TH + (strip >> 2), ox0 = tx * ENC_DW_TW + (strip & 3) * 4;
    const bool live = c < p.c_pad && oy < p.ho && ox0 < p.wo;
    float psum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
        float acc[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
        constexpr int SPAN = 3 * S + K;                       // input pixels of one window row that the 4 outputs touch
        const int ix0 = ox0 * S - p.pad_left;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = oy * S + ky - p.pad_top;
            if (iy < 0 || iy >= p.hi) continue;
            float wk[K][8];
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const float4 a = *reinterpret_cast<const float4*>(p.wgt + (size_t)(ky * K + kx) * p.c_pad + c);
                const float4 b = *reinterpret_cast<const float4*>(p.wgt + (size_t)(ky * K + kx) * p.c_pad + c + 4);
                wk[kx][0] = a.x; wk[kx][1] = a.y; wk[kx][2] = a.z; wk[kx][3] = a.w;
                wk[kx][4] = b.x; wk[kx][5] = b.y; wk[kx][6] = b.z; wk[kx][7] = b.w;
            }
            const size_t rowbase = ((size_t)n * (p.hi + 2) + (iy + 1)) * (p.wi + 2) + 1;
#pragma unroll
            for (int t = 0; t < SPAN; ++t) {
                const int ix = ix0 + t;
                if (ix < 0 || ix >= p.wi) continue;
                float v[8];
                ek_load8<F16>(p.in_hi, p.in_lo, (rowbase + ix) * p.in_ld + c, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kx = t - j * S;                 // compile-time after unrolling
                    if (kx >= 0 && kx < K) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[j][i] = __builtin_fmaf(wk[kx][i], v[i], acc[j][i]);
                    }
                }
            }
        }
        const float4 b0 = *reinterpret_cast<const float4*>(p.bias + c), b1 = *reinterpret_cast<const float4*>(p.bias + c + 4);
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        const size_t orow = ((size_t)n * (p.ho + 2) + (oy + 1)) * (p.wo + 2) + 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ox0 + j >= p.wo) continue;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[i] = silu_f32(acc[j][i] + bv[i]);
                psum[i] += v[i];
            }
            ek_store8<F16>(p.out_hi, p.out_lo, (orow + ox0 + j) * p.out_ld + c, v);
        }
    }
    const int cw = cgb * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) red[strip * cw + g * 8 + i] = psum[i];
    __syncthreads();
    if (threadIdx.x < cw) {
        const int ch = blockIdx.y * cw + threadIdx.x;
        if (ch < p.c_pad) {
            float s = red[threadIdx.x];
            for (int k = 1; k < 32; ++k) s += red[k * cw + threadIdx.x];
            p.part[((size_t)n * p.n_part + tile) * p.c_pad + ch] = s;
        }
    }
}

template <bool F16>
static hipError_t launch_enc_dwconv_fmt(const EncDwParams& p_in, int N, hipStream_t s) {
    EncDwParams p = p_in;
    p.n_part = (int)enc_dw_parts(p.ho, p.wo);
    const int groups = p.c_pad / 8;
    const int cgb = (groups % 8) == 0 ? 8 : 4;                // c_pad % 32 == 0: groups is a multiple of 4
    const dim3 grid((unsigned)p.n_part, (unsigned)(groups / cgb), (unsigned)N), block(32 * cgb);
    const size_t lds = (size_t)32 * cgb * 8 * sizeof(float);
    if (p.k == 3 && p.stride == 1) hipLaunchKernelGGL((enc_dwconv_kernel<3, 1, F16>), grid, block, lds, s, p);
    else if (p.k == 3 && p.stride == 2) hipLaunchKernelGGL((enc_dwconv_kernel<3, 2, F16>), grid, block, lds, s, p);
    else if (p.k == 5 && p.stride == 1) hipLaunchKernelGGL((enc_dwconv_kernel<5, 1, F16>), grid, block, lds, s, p);
    else if (p.k == 5 && p.stride == 2) hipLaunchKernelGGL((enc_dwconv_kernel<5, 2, F16>), grid, block, lds, s, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// f16: in_hi / out_hi are fp16 planes and the lo pointers NULL (magnet_dwconv_cl_f16)
hipError_t launch_enc_dwconv(const EncDwParams& p, int N, bool f16, hipStream_t s) {
    return f16 ? launch_enc_dwconv_fmt<true>(p, N, s) : launch_enc_dwconv_fmt<false>(p, N, s);
}

// ---- squeeze-excite gate: one workgroup of 1024 threads per image ----
// The launch is latency-bound (a few hundred KB of weights, one workgroup), so every phase keeps many independent loads in flight:
// mean   the partials (n_part rows of c_pad floats, contiguous) are copied to LDS in chunks by all threads (coalesced 16-byte loads);
//        thread c then adds its channel's values of the chunk in ascending row order: mean[c] = (((p0 + p1) + p2) + ...) * fl(1 / hw)
// reduce r[j] = silu(b1[j] + sum_c w1[j][c] mean[c]): one wave per j; lane l takes the channel quads 4 (l + 64 i) .. + 3, i ascending,
//        as 4 fused multiply-adds each in channel order (a tail of C % 4 channels goes to lanes 0 .. 2), then the 64 lane sums are
//        added by a butterfly of 6 steps (a fixed tree)
// expand gate[c] = sigmoid(b2[c] + sum_j w2t[j][c] r[j]), j ascending, one thread per channel (coalesced over c)
// Deterministic: no atomics, every order is fixed.
constexpr int ENC_GATE_THREADS = 1024;
constexpr int ENC_GATE_STAGE = 8192;                          // floats of the LDS staging buffer (>= c_pad: the API checks C <= 8192)

__global__ __launch_bounds__(ENC_GATE_THREADS) void enc_se_gate_kernel(const float* __restrict__ part, int n_part, float inv_hw,
                                                                       const float* __restrict__ w1, const float* __restrict__ b1,
                                                                       const float* __restrict__ w2t, const float* __restrict__ b2, int C, int R,
                                                                       int c_pad, float* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) float sm[];         // stage[ENC_GATE_STAGE], mean[round_up(C, 4)], r[R]
    float* stage = sm;
    float* mean = sm + ENC_GATE_STAGE;
    float* r = mean + ((C + 3) & ~3);
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* src = part + (size_t)n * n_part * c_pad;
    const int rows_per = ENC_GATE_STAGE / c_pad;               // >= 1; c_pad % 32 == 0, so a chunk is a whole number of float4
    for (int c = tid; c < C; c += ENC_GATE_THREADS) mean[c] = 0.f;
    for (int k0 = 0; k0 < n_part; k0 += rows_per) {
        const int nk = (n_part - k0 < rows_per) ? n_part - k0 : rows_per;
        const int quads = nk * c_pad / 4;
        const float4* s4 = reinterpret_cast<const float4*>(src + (size_t)k0 * c_pad);
        __syncthreads();                                      // the previous chunk has been consumed (and mean[] is initialised)
        for (int q = tid; q < quads; q += ENC_GATE_THREADS) reinterpret_cast<float4*>(stage)[q] = s4[q];
        __syncthreads();
        for (int c = tid; c < C; c += ENC_GATE_THREADS) {
            float s = mean[c];
            for (int k = 0; k < nk; ++k) s += stage[k * c_pad + c];
            mean[c] = s;
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += ENC_GATE_THREADS) mean[c] *= inv_hw;
    __syncthreads();
    const int C4 = C & ~3;
    const bool w_vec = (C & 3) == 0;                          // rows of w1 are 16-byte aligned only then
    for (int j = wv; j < R; j += ENC_GATE_THREADS / 64) {
        const float* wj = w1 + (size_t)j * C;
        float s = 0.f;
        for (int c = lane * 4; c < C4; c += 256) {
            float4 w;
            if (w_vec) w = *reinterpret_cast<const float4*>(wj + c);
            else w = make_float4(wj[c], wj[c + 1], wj[c + 2], wj[c + 3]);
            const float4 m = *reinterpret_cast<const float4*>(mean + c);
            s = __builtin_fmaf(w.x, m.x, s); s = __builtin_fmaf(w.y, m.y, s); s = __builtin_fmaf(w.z, m.z, s); s = __builtin_fmaf(w.w, m.w, s);
        }
        if (C4 + lane < C) s = __builtin_fmaf(wj[C4 + lane], mean[C4 + lane], s);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) r[j] = silu_f32(s + b1[j]);
    }
    __syncthreads();
    for (int c = tid; c < c_pad; c += ENC_GATE_THREADS) {
        float gv = 0.f;
        if (c < C) {
            float s = 0.f;
#pragma unroll 8
            for (int j = 0; j < R; ++j) s = __builtin_fmaf(w2t[(size_t)j * C + c], r[j], s);
            gv = sigmoid_f32(s + b2[c]);
        }
        gate[(size_t)n * c_pad + c] = gv;
    }
}

hipError_t launch_enc_se_gate(const float* part, int n_part, long long hw, const float* w1, const float* b1, const float* w2t, const float* b2,
                              int C, int R, int c_pad, float* gate, int N, hipStream_t s) {
    const size_t lds = (size_t)(ENC_GATE_STAGE + ((C + 3) & ~3) + R) * sizeof(float);      // <= 8192 + 8192 + 1024 floats = 68 KiB
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(enc_se_gate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(enc_se_gate_kernel, dim3((unsigned)N), dim3(ENC_GATE_THREADS), lds, s, part, n_part, 1.0f / (float)hw, w1, b1, w2t, b2, C, R,
                       c_pad, gate);
    return hipGetLastError();
}

// ---- squeeze-excite scale: out = split((hi + lo) * gate[n][c]) over the interior; one thread per (pixel, 8 channels) ----
// F16: out = f16(in * gate[n][c]) on ONE fp16 plane (magnet_se_scale_f16); in place is allowed either way (one reader = the one writer)
template <bool F16>
__global__ __launch_bounds__(256) void enc_se_scale_kernel(const uint16_t* __restrict__ in_hi, const uint16_t* __restrict__ in_lo, int in_ld,
                                                           const float* __restrict__ gate, int N, int h, int w, int c_pad,
                                                           uint16_t* __restrict__ out_hi, uint16_t* __restrict__ out_lo, int out_ld) {
    const int groups = c_pad / 8;
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long pix = it / groups;
    if (pix >= (long long)N * h * w) return;
    const int c = (int)(it - pix * groups) * 8;
    const int x = (int)(pix % w), y = (int)((pix / w) % h), n = (int)(pix / ((long long)w * h));
    const size_t row = ((size_t)n * (h + 2) + (y + 1)) * (w + 2) + (x + 1);
    float v[8];
    ek_load8<F16>(in_hi, in_lo, row * in_ld + c, v);
    const float4 g0 = *reinterpret_cast<const float4*>(gate + (size_t)n * c_pad + c), g1 = *reinterpret_cast<const float4*>(gate + (size_t)n * c_pad + c + 4);
    const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] *= gv[i];
    ek_store8<F16>(out_hi, out_lo, row * out_ld + c, v);
}

hipError_t launch_enc_se_scale(const uint16_t* in_hi, const uint16_t* in_lo, int in_ld, const float* gate, int N, int h, int w, int c_pad,
                               uint16_t* out_hi, uint16_t* out_lo, int out_ld, bool f16, hipStream_t s) {
    const long long items = (long long)N * h * w * (c_pad / 8);
    const dim3 grid((unsigned)((items + 255) / 256));
    if (f16) hipLaunchKernelGGL(enc_se_scale_kernel<true>, grid, dim3(256), 0, s, in_hi, nullptr, in_ld, gate, N, h, w, c_pad, out_hi, nullptr, out_ld);
    else hipLaunchKernelGGL(enc_se_scale_kernel<false>, grid, dim3(256), 0, s, in_hi, in_lo, in_ld, gate, N, h, w, c_pad, out_hi, out_lo, out_ld);
    return hipGetLastError();
}

}  // namespace magnet
