// pack_tile.hpp — what the wide layout packs share (conv_mfma.hip: pack_split_wide_kernel, pack_mx_kernel; elementwise.hip:
// pack_wide_kernel): the 128-pixel x 64-channel LDS tile and its streaming global accesses.
//
// A pack reads every source element once and writes every destination element once, so its 16-byte loads and stores are marked
// non-temporal (PACK_STREAM).  At 64 frames of 120 x 160 on one MI355X: x_d3 pack 0.469 -> 0.448 ms, source features
// 0.329 -> 0.308 ms, reference features 0.083 -> 0.074 ms (profiles/pack_phase/NOTES.md).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace magnet {

constexpr bool PACK_STREAM = true;

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

// 128 pixels x 64 channels per workgroup of 256 threads, 8 independent 16-byte loads per thread (512-byte runs along the pixel
// axis), tile rows of 132 floats with the pixel index XOR-swizzled in 4-word blocks by the channel octet: the float4 tile writes and
// the transposed channel reads (8 lanes = one pixel's 8 octets) are both conflict-free.
constexpr int PW_PIX = 128, PW_S = 132;
__device__ __forceinline__ int pw_idx(int c, int q) { return c * PW_S + (q ^ (((c >> 3) & 7) << 2)); }

// channels [f0, f0 + 64) of pixels [p0, p0 + 128) of one image (`src` = its channel 0, pixel 0; C channels of hw pixels,
// hw % 4 == 0) into the tile; zeros where the image or the channels end.  The caller synchronises before it reads the tile.
template <bool NT>
__device__ __forceinline__ void pw_fill_tile(float* __restrict__ tile, const float* __restrict__ src, int C, int hw, int p0, int f0) {
    const int tid = threadIdx.x, l4 = (tid & 31) * 4, cr = tid >> 5;          // 32 lanes x float4 = one channel row of the tile
    float4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int f = f0 + cr + 8 * k, pp = p0 + l4;
        v[k] = (pp < hw && f < C) ? pk_load4<NT>(src + (size_t)f * hw + pp) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(&tile[pw_idx(cr + 8 * k, l4)]) = v[k];
}

}  // namespace magnet
