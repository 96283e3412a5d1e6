// pack.hip — every NCHW fp32 -> channel-last layout pack, as one kernel template, and the planes -> fp16 conversion next to it.
//
// pack_nchw_kernel<Fmt, PIX>: a workgroup of 256 threads moves PIX pixels x 64 channels of one image through an LDS tile (global reads
// run along the pixel axis, global writes are 16-byte vectors along the channel axis) into channels [c_off, c_off + C) of the interior
// of a channel-last buffer (N, h + 2 pad, w + 2 pad, ctot).  The border and the other channels are not touched.  Whole vectors of
// Fmt::VEC channels are written: where C ends inside one, the round-up lanes are +0.  What differs between the packs is only what one
// 16-byte store holds, which is Fmt:
//
//   Fmt    entry point                        VEC  STREAM  PAD  one vector of VEC channels becomes
//   F32    magnet_pack_features (fp32)          4  yes     -1   16 bytes of fp32
//   BF16   magnet_pack_features (bf16)          8  yes     -1   16 bytes of bf16 (round to nearest even)
//   SPLIT  magnet_pack_split                    8  yes      1   16 bytes in the hi plane + 16 in the lo plane (split_bf16x2)
//   F16    magnet_pack_f16                      8  no       1   16 bytes of saturated fp16 (f16x2_bits_sat)
//
// PAD is the destination border as a compile-time constant, -1 where the caller chooses it at run time.
// STREAM marks the 16-byte loads and stores of the wide form non-temporal: a pack reads every source element once and writes every
// destination element once.  At 64 frames of 120 x 160 on one MI355X: x_d3 pack 0.469 -> 0.448 ms, source features 0.329 -> 0.308 ms,
// reference features 0.083 -> 0.074 ms; it is no gain for small or cache-resident packs, which is why F16 stays without
// (profiles/pack_phase/NOTES.md §1 and §5).
//
// The fp16 conversion (F16 and planes_to_f16): round to nearest even; a magnitude that would round above 65504 (+-Inf included)
// becomes +-65504; NaN is written through; the sign of zero is kept.  tests/test_conv_precision_host.py
// restates it in numpy and the GPU tests compare bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "warp_math.hpp"
#include "conv_common.hpp"                                   // f16x2_bits_sat
#include "pack.hpp"

namespace magnet {

typedef float pk_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t pk_u32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ float4 pk_load4(const float* p) {
    if constexpr (NT) {
        const pk_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const pk_f32x4*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return *reinterpret_cast<const float4*>(p);
    }
}

template <bool NT>
__device__ __forceinline__ void pk_store4(void* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    if constexpr (NT) {
        pk_u32x4 v; v.x = a; v.y = b; v.z = c; v.w = d;
        __builtin_nontemporal_store(v, reinterpret_cast<pk_u32x4*>(p));
    } else {
        *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d);
    }
}

// ---- the formats: store<NT>(row, ctot, ch, v) writes channels [ch, ch + VEC) of destination row `row`; v(k) is the tile's value of
// ---- channel ch + k, read from LDS when the format asks for it ----
struct PackF32 {
    float* out;
    static constexpr int VEC = 4;
    static constexpr int PAD = -1;                            // the features' border is the caller's: 0 or 1 at run time
    static constexpr bool STREAM = true;
    template <bool NT, class V> __device__ __forceinline__ void store(size_t row, int ctot, int ch, const V& v) const {
        pk_store4<NT>(out + row * ctot + ch, __float_as_uint(v(0)), __float_as_uint(v(1)), __float_as_uint(v(2)), __float_as_uint(v(3)));
    }
};

struct PackBF16 {
    uint16_t* out;
    static constexpr int VEC = 8, PAD = -1;
    static constexpr bool STREAM = true;
    template <bool NT, class V> __device__ __forceinline__ void store(size_t row, int ctot, int ch, const V& v) const {
        uint32_t wd[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wd[k] = f32x2_to_bf16x2_rne(v(2 * k), v(2 * k + 1));
        pk_store4<NT>(out + row * ctot + ch, wd[0], wd[1], wd[2], wd[3]);
    }
};

struct PackSplit {
    uint16_t* hi; uint16_t* lo;
    static constexpr int VEC = 8, PAD = 1;
    static constexpr bool STREAM = true;
    template <bool NT, class V> __device__ __forceinline__ void store(size_t row, int ctot, int ch, const V& v) const {
        uint32_t hh[4], ll[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) split_bf16x2(v(2 * k), v(2 * k + 1), hh[k], ll[k]);
        const size_t e = row * ctot + ch;
        pk_store4<NT>(hi + e, hh[0], hh[1], hh[2], hh[3]);
        pk_store4<NT>(lo + e, ll[0], ll[1], ll[2], ll[3]);
    }
};

struct PackF16 {
    uint16_t* out;
    static constexpr int VEC = 8, PAD = 1;
    static constexpr bool STREAM = false;
    template <bool NT, class V> __device__ __forceinline__ void store(size_t row, int ctot, int ch, const V& v) const {
        uint32_t hh[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) hh[k] = f16x2_bits_sat(v(2 * k), v(2 * k + 1));
        pk_store4<NT>(out + row * ctot + ch, hh[0], hh[1], hh[2], hh[3]);
    }
};

// ---- the tile: [64 channels][PIX pixels] ----
// PIX = 128, the wide form: 8 independent 16-byte loads per thread (512-byte runs along the pixel axis), tile rows of 132 floats with
// the pixel index XOR-swizzled in 4-word blocks by the channel octet: the float4 tile writes and the transposed channel reads (8 lanes
// = one pixel's 8 octets) are both conflict-free.  33 792 B.
// PIX = 64, the narrow form, for sources the float4 loads cannot read: scalar loads, rows of 65 floats, plain stores.  16 640 B.
constexpr int PW_S = 132, PN_S = 65;
template <int PIX>
__device__ __forceinline__ int pk_idx(int c, int q) {
    if constexpr (PIX == 128) return c * PW_S + (q ^ (((c >> 3) & 7) << 2));
    else return c * PN_S + q;
}

// channels [f0, f0 + 64) of pixels [p0, p0 + PIX) of one image (`src` = its channel 0, pixel 0; C channels of hw pixels; wide:
// hw % 4 == 0 and src 16-byte aligned) into the tile; zeros where the image or the channels end.  The caller synchronises.
template <int PIX, bool NT>
__device__ __forceinline__ void pk_fill_tile(float* __restrict__ tile, const float* __restrict__ src, int C, int hw, int p0, int f0) {
    const int tid = threadIdx.x;
    if constexpr (PIX == 128) {
        const int l4 = (tid & 31) * 4, cr = tid >> 5;                         // 32 lanes x float4 = one channel row of the tile
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int f = f0 + cr + 8 * k, pp = p0 + l4;
            v[k] = (pp < hw && f < C) ? pk_load4<NT>(src + (size_t)f * hw + pp) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(&tile[pk_idx<PIX>(cr + 8 * k, l4)]) = v[k];
    } else {
        const int px = tid & 63, cs = tid >> 6, pp = p0 + px;
        for (int c = cs; c < 64; c += 4) {
            const int f = f0 + c;
            tile[pk_idx<PIX>(c, px)] = (pp < hw && f < C) ? src[(size_t)f * hw + pp] : 0.f;
        }
    }
}

struct PackGeom {
    int C, h, w;                                              // the source: C channels of h x w pixels per image,
    long long in_img_stride;                                  // images this many floats apart
    int ctot, c_off, pad;                                     // the destination: rows of ctot channels, ours from c_off; border width
                                                              // (read only by the formats whose PAD is -1)
};

// 1-D grid with the channel group as the fastest index: the workgroups that write one destination row's channel run (128 bytes each
// per plane) are neighbours in dispatch order, not a quarter of the launch apart as with the channel group in grid.y (x_d3 of 64
// frames: 0.483 -> 0.469 ms; with the streaming accesses 0.448 ms).  One workgroup per row run was measured and is slower: looping
// over 4 groups 0.469 ms, a 32-pixel x 256-channel tile 0.484 ms, 64 x 128 0.459 ms, all streaming (profiles/pack_phase/NOTES.md).
template <class Fmt, int PIX>
__global__ __launch_bounds__(256) void pack_nchw_kernel(const float* __restrict__ in, const Fmt fmt, const PackGeom g) {
    __shared__ __attribute__((aligned(16))) float tile[64 * (PIX == 128 ? PW_S : PN_S)];
    constexpr bool NT = Fmt::STREAM && PIX == 128;
    const int hw = g.h * g.w;
    const int bpi = (hw + PIX - 1) / PIX, ng = (g.C + 63) / 64;
    const int pt = blockIdx.x / ng, f0 = (blockIdx.x - pt * ng) * 64;
    const int n = pt / bpi, p0 = (pt - n * bpi) * PIX;
    const int tid = threadIdx.x;
    pk_fill_tile<PIX, NT>(tile, in + (size_t)n * g.in_img_stride, g.C, hw, p0, f0);
    __syncthreads();
    constexpr int VEC = Fmt::VEC, VPP = 64 / VEC;             // channels per store, stores per pixel
    const int pad = Fmt::PAD >= 0 ? Fmt::PAD : g.pad;         // a constant where the format has one: the parent kernels' arithmetic
#pragma unroll
    for (int it = 0; it < PIX * VPP / 256; ++it) {
        const int i = tid + it * 256;
        const int q = i / VPP, vc = (i % VPP) * VEC, pq = p0 + q;
        if (pq >= hw || f0 + vc >= g.C) continue;
        const int y = pq / g.w, x = pq - y * g.w;
        const size_t row = ((size_t)n * (g.h + 2 * pad) + (y + pad)) * (g.w + 2 * pad) + (x + pad);
        fmt.template store<NT>(row, g.ctot, g.c_off + f0 + vc, [&](int k) { return tile[pk_idx<PIX>(vc + k, q)]; });
    }
}

// The one launcher.  Wide where the float4 loads can read the source, else narrow; the dev library's MAGNET_PACK_NARROW (read once
// per process, pack_force_narrow) forces narrow for A/B runs.
static bool pack_force_narrow() {
#ifdef MAGNET_DEV
    static const bool narrow = getenv("MAGNET_PACK_NARROW") != nullptr;      // dev A/B: the 64-pixel kernel
    return narrow;
#else
    return false;
#endif
}

template <class Fmt>
static hipError_t launch_pack_nchw(const float* in, const Fmt& fmt, int N, const PackGeom& g, hipStream_t s) {
    const bool narrow = pack_force_narrow();
    const int hw = g.h * g.w;
    const bool wide = !narrow && hw % 4 == 0 && g.C % 8 == 0 && g.in_img_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const int pix = wide ? 128 : 64;
    const long long blocks = (long long)N * ((hw + pix - 1) / pix) * ((g.C + 63) / 64);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (wide) hipLaunchKernelGGL((pack_nchw_kernel<Fmt, 128>), dim3((unsigned)blocks), dim3(256), 0, s, in, fmt, g);
    else hipLaunchKernelGGL((pack_nchw_kernel<Fmt, 64>), dim3((unsigned)blocks), dim3(256), 0, s, in, fmt, g);
    return hipGetLastError();
}

// zero the one-texel border of (N, h+2, w+2, F) images: 16-byte vectors
__global__ __launch_bounds__(256) void zero_border_kernel(uint4* __restrict__ out, int N, int h, int w, int vec_per_tex) {
    const int Wp = w + 2, Hp = h + 2;
    const int per_img = 2 * Wp + 2 * h;                      // border texels of one image
    const size_t total = (size_t)N * per_img * vec_per_tex;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % vec_per_tex);
        const size_t t = i / vec_per_tex;
        const int n = (int)(t / per_img), k = (int)(t % per_img);
        int y, x;
        if (k < Wp) { y = 0; x = k; }
        else if (k < 2 * Wp) { y = Hp - 1; x = k - Wp; }
        else { const int m = k - 2 * Wp; y = 1 + (m >> 1); x = (m & 1) ? Wp - 1 : 0; }
        out[(((size_t)n * Hp + y) * Wp + x) * vec_per_tex + c] = make_uint4(0, 0, 0, 0);
    }
}

hipError_t launch_pack(const float* in, void* out, int N, int F, int h, int w, bool bf16, int pad, hipStream_t s) {
    if (pad) {
        const int vec_per_tex = F * (bf16 ? 2 : 4) / 16;
        const size_t total = (size_t)N * (2 * (w + 2) + 2 * h) * vec_per_tex;
        const unsigned nb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(zero_border_kernel, dim3(nb), dim3(256), 0, s, reinterpret_cast<uint4*>(out), N, h, w, vec_per_tex);
    }
    const PackGeom g{F, h, w, (long long)F * h * w, F, 0, pad};
    return bf16 ? launch_pack_nchw(in, PackBF16{(uint16_t*)out}, N, g, s) : launch_pack_nchw(in, PackF32{(float*)out}, N, g, s);
}

hipError_t launch_pack_split(const float* in, uint16_t* out_hi, uint16_t* out_lo, int N, int C, int h, int w, int ctot, int c_off,
                             long long in_img_stride, hipStream_t s) {
    return launch_pack_nchw(in, PackSplit{out_hi, out_lo}, N, PackGeom{C, h, w, in_img_stride, ctot, c_off, 1}, s);
}

hipError_t launch_pack_f16(const float* in, uint16_t* out, int N, int C, int h, int w, int ctot, int c_off, long long in_img_stride,
                           hipStream_t s) {
    return launch_pack_nchw(in, PackF16{out}, N, PackGeom{C, h, w, in_img_stride, ctot, c_off, 1}, s);
}

// ---- split-bf16 planes (rows, ld), channels [c0, c0 + 8 nv) -> the same channels of an fp16 plane (rows, ld16): f16(hi + lo), the sum
// ---- in fp32.  One thread = one 8-channel vector of one row: two 16-byte loads, one 16-byte store; consecutive threads walk a row's
// ---- vectors, so a wave touches whole 128-byte lines wherever the channel range is 64-aligned.
__global__ __launch_bounds__(256) void planes_to_f16_kernel(const uint16_t* __restrict__ in_hi, const uint16_t* __restrict__ in_lo,
                                                             uint16_t* __restrict__ out, long long rows, int ld, int ld16, int c0, int nv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * nv) return;
    const long long row = i / nv;
    const int ch = c0 + (int)(i - row * nv) * 8;
    const uint4 h4 = *reinterpret_cast<const uint4*>(in_hi + row * ld + ch);
    const uint4 l4 = *reinterpret_cast<const uint4*>(in_lo + row * ld + ch);
    const uint32_t hw_[4] = {h4.x, h4.y, h4.z, h4.w}, lw_[4] = {l4.x, l4.y, l4.z, l4.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float a = __uint_as_float(hw_[k] << 16) + __uint_as_float(lw_[k] << 16);
        const float b = __uint_as_float(hw_[k] & 0xffff0000u) + __uint_as_float(lw_[k] & 0xffff0000u);
        o[k] = f16x2_bits_sat(a, b);
    }
    *reinterpret_cast<uint4*>(out + row * ld16 + ch) = make_uint4(o[0], o[1], o[2], o[3]);
}

hipError_t launch_planes_to_f16(const uint16_t* in_hi, const uint16_t* in_lo, uint16_t* out, long long rows, int ld, int ld16, int c0, int c1,
                                hipStream_t s) {
    const int nv = (c1 - c0) / 8;
    const long long blocks = (rows * nv + 255) / 256;
    hipLaunchKernelGGL(planes_to_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in_hi, in_lo, out, rows, ld, ld16, c0, nv);
    return hipGetLastError();
}

}  // namespace magnet
