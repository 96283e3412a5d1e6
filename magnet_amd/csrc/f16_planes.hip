// f16_planes.hip — the two element-wise kernels that fill the single-plane fp16 activation buffer of magnet_conv_mfma_f16
// (include/magnet_hip.h): magnet_pack_f16 (fp32 NCHW -> fp16 channel-last interior) and magnet_planes_to_f16 (split-bf16 planes ->
// fp16 plane, same rows and channels).  Both are HBM-bound copies with a conversion; ordinary vector loads and stores.
//
// The conversion, in both: round to nearest even; a magnitude that would round above 65504 (+-Inf included) becomes +-65504, as
// magnet_pack_mx clamps its fp16 plane; NaN is written through; the sign of zero is kept.  tests/test_conv_precision_host.py restates
// it in numpy and the GPU tests compare bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_common.hpp"

namespace magnet {

// f16_bits_sat / f16x2_bits_sat: conv_common.hpp (shared with the convolution epilogue and the F-Net's small kernels)

// ---- fp32 NCHW (N, C, h, w) -> fp16 plane of the padded channel-last buffer (N, h+2, w+2, ctot), channels [c_off, c_off + C);
// ---- 64 pixels x 64 channels per block through LDS; interior only (pack_split_kernel's structure, one output plane)
__global__ __launch_bounds__(256) void pack_f16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int C, int h, int w,
                                                        int ctot, int c_off, long long in_img_stride) {
    __shared__ float tile[64][65];
    const int hw = h * w;
    const int bpi = (hw + 63) / 64;
    const int n = blockIdx.x / bpi, p0 = (blockIdx.x % bpi) * 64, f0 = blockIdx.y * 64;
    const int tid = threadIdx.x, px = tid & 63, cs = tid >> 6;
    for (int c = cs; c < 64; c += 4) {
        const int f = f0 + c, pp = p0 + px;
        tile[c][px] = (pp < hw && f < C) ? in[(size_t)n * in_img_stride + (size_t)f * hw + pp] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < 64 * 8; i += 256) {                 // 64 pixels x 8 vectors of 8 channels
        const int q = i >> 3, vc = (i & 7) * 8, pq = p0 + q;
        if (pq >= hw || f0 + vc >= C) continue;
        const int y = pq / w, x = pq % w;
        const size_t row = ((size_t)n * (h + 2) + (y + 1)) * (w + 2) + (x + 1);
        uint32_t hh[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) hh[k] = f16x2_bits_sat(tile[vc + 2 * k][q], tile[vc + 2 * k + 1][q]);
        *reinterpret_cast<uint4*>(out + row * ctot + c_off + f0 + vc) = make_uint4(hh[0], hh[1], hh[2], hh[3]);
    }
}

// Wide variant (h*w % 4 == 0, C % 8 == 0): pack_split_wide_kernel's tile — 128 pixels x 64 channels per workgroup, 8 independent
// 16-byte loads per thread, tile rows of 132 floats with the pixel index XOR-swizzled in 4-word blocks by the channel octet, so the
// float4 tile writes and the transposed channel reads are both conflict-free.
constexpr int PF_PIX = 128, PF_S = 132;
__device__ __forceinline__ int pf_idx(int c, int q) { return c * PF_S + (q ^ (((c >> 3) & 7) << 2)); }
__global__ __launch_bounds__(256) void pack_f16_wide_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int C, int h, int w,
                                                             int ctot, int c_off, long long in_img_stride) {
    __shared__ __attribute__((aligned(16))) float tile[64 * PF_S];
    const int hw = h * w;
    const int bpi = (hw + PF_PIX - 1) / PF_PIX;
    const int n = blockIdx.x / bpi, p0 = (blockIdx.x % bpi) * PF_PIX, f0 = blockIdx.y * 64;
    const int tid = threadIdx.x, l4 = (tid & 31) * 4, cr = tid >> 5;          // 32 lanes x float4 = one channel row of the tile
    float4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = cr + 8 * k, f = f0 + c, pp = p0 + l4;
        v[k] = (pp < hw && f < C) ? *reinterpret_cast<const float4*>(in + (size_t)n * in_img_stride + (size_t)f * hw + pp)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(&tile[pf_idx(cr + 8 * k, l4)]) = v[k];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {                          // 128 pixels x 8 octets
        const int i = tid + it * 256;
        const int q = i >> 3, vc = (i & 7) * 8, pq = p0 + q;
        if (pq >= hw || f0 + vc >= C) continue;
        const int y = pq / w, x = pq - y * w;
        const size_t row = ((size_t)n * (h + 2) + (y + 1)) * (w + 2) + (x + 1);
        uint32_t hh[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) hh[k] = f16x2_bits_sat(tile[pf_idx(vc + 2 * k, q)], tile[pf_idx(vc + 2 * k + 1, q)]);
        *reinterpret_cast<uint4*>(out + row * ctot + c_off + f0 + vc) = make_uint4(hh[0], hh[1], hh[2], hh[3]);
    }
}

hipError_t launch_pack_f16(const float* in, uint16_t* out, int N, int C, int h, int w, int ctot, int c_off, long long in_img_stride,
                           hipStream_t s) {
    // the wide kernel under launch_pack_split's conditions, else the 64-pixel one
    if ((h * w) % 4 == 0 && C % 8 == 0 && in_img_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0) {
        const int bpw = (h * w + PF_PIX - 1) / PF_PIX;
        hipLaunchKernelGGL(pack_f16_wide_kernel, dim3((unsigned)(N * bpw), (unsigned)((C + 63) / 64)), dim3(256), 0, s, in, out, C, h, w, ctot,
                           c_off, in_img_stride);
        return hipGetLastError();
    }
    const int bpi = (h * w + 63) / 64;
    hipLaunchKernelGGL(pack_f16_kernel, dim3((unsigned)(N * bpi), (unsigned)((C + 63) / 64)), dim3(256), 0, s, in, out, C, h, w, ctot, c_off,
                       in_img_stride);
    return hipGetLastError();
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
