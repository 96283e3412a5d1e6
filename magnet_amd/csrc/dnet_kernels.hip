// dnet_kernels.hip — the part of MaGNet's D-Net decoder (DenseDepth_BN at downsample ratio 4, reference
// models/submodules/D_dense_depth.py:104-195, models/DNET.py:62-67) that is not a matrix-core convolution.
// The convolutions (conv2, up1..up3 with folded BatchNorm + LeakyReLU, the depth head) run on conv_mfma_kernel
// (magnet_conv_mfma_ex); the bilinear upsampling and the skip concatenation on the F-Net's kernels
// (magnet_upsample_bilinear_cl, magnet_pack_split).  What is left is the Gaussian activation behind the depth head, and for the
// stand-alone D-Net (DNET(dnet=True), D_dense_depth.py:85-100,187-192 + DNET.py:55-60) the learned convex upsampling with the
// activation behind it.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace magnet {

namespace {

// activation_G_magnet (DNET.py:62-67): out (N, 2, h, w) = [o0, sqrt(elu(o1) + 1 + 1e-10)] of the depth head's fp32 output
// (rows, in_ld) over zero-bordered (N, h+2*pad, w+2*pad) grids, channels 0 and 1; border rows are not read.
__global__ __launch_bounds__(256) void dnet_gauss_head_kernel(const float* __restrict__ in, int in_ld, int N, int h, int w, int pad,
                                                              float* __restrict__ out) {
    const long long hw = (long long)h * w;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * hw) return;
    const long long n = idx / hw;
    const int r = (int)(idx - n * hw);
    const int y = r / w, x = r - (r / w) * w;
    const size_t row = ((size_t)n * (h + 2 * pad) + (y + pad)) * (size_t)(w + 2 * pad) + (x + pad);
    const float2 o = *reinterpret_cast<const float2*>(in + row * in_ld);
    const float e = (o.y > 0.f) ? o.y : expm1f(o.y);                  // F.elu
    const float var = (e + 1.0f) + 1e-10f;                             // DNET.py:64, in the reference's order
    out[(size_t)n * 2 * hw + r] = o.x;
    out[(size_t)n * 2 * hw + hw + r] = sqrtf(var);                     // correctly rounded (build flag), as torch.sqrt
}

// The stand-alone D-Net's tail in one pass (D_dense_depth.py:85-100 then DNET.py:55-60): out (N, 2, 4h, 4w) =
// [up(mu), elu(up(v)) + 1 + 1e-10], up = the convex combination of the 3x3 neighbourhood of the RAW head output under the softmax of
// the mask head's 9 logits per sub-pixel.  Both inputs are the convolution kernel's fp32 output over (N, h+2, w+2) grids: head
// (rows, head_ld) with channel 0 = mu, 1 = v; mask (rows, mask_ld) with channel n*16 + i*4 + j.  Thread = (coarse pixel, sub-row i):
// for a fixed tap n the 4 sub-columns j are 16 contiguous bytes, and the 4 outputs of a sub-row are one 16-byte store per channel.
// Neighbours outside the image count as zero (F.unfold(padding=1)); they are decided by index, so the border rows of `head`, where the
// convolution kernel leaves whatever its taps gave, are never read.
__global__ __launch_bounds__(256) void dnet_upsample_gauss_kernel(const float* __restrict__ head, int head_ld,
                                                                   const float* __restrict__ mask, int mask_ld, int N, int h, int w,
                                                                   float* __restrict__ out) {
    const size_t hw = (size_t)h * w;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)N * hw * 4) return;
    const int i = (int)(t & 3);
    const size_t pi = t >> 2, b = pi / hw, pp = pi % hw;
    const int y = (int)(pp / w), x = (int)(pp % w);
    const size_t row = ((size_t)b * (h + 2) + (y + 1)) * (w + 2) + (x + 1);
    const float* m = mask + row * mask_ld + i * 4;
    float4 mv[9];
    float4 mx = make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        mv[n] = *reinterpret_cast<const float4*>(m + n * 16);
        mx.x = fmaxf(mx.x, mv[n].x); mx.y = fmaxf(mx.y, mv[n].y); mx.z = fmaxf(mx.z, mv[n].z); mx.w = fmaxf(mx.w, mv[n].w);
    }
    float4 den = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        mv[n].x = expf(mv[n].x - mx.x); mv[n].y = expf(mv[n].y - mx.y);
        mv[n].z = expf(mv[n].z - mx.z); mv[n].w = expf(mv[n].w - mx.w);
        den.x += mv[n].x; den.y += mv[n].y; den.z += mv[n].z; den.w += mv[n].w;
    }
    const float4 inv = make_float4(1.0f / den.x, 1.0f / den.y, 1.0f / den.z, 1.0f / den.w);
    float4 amu = make_float4(0.f, 0.f, 0.f, 0.f), av = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const int dy = n / 3 - 1, dx = n % 3 - 1;
        const int yy = y + dy, xx = x + dx;
        float2 o = make_float2(0.f, 0.f);
        if (yy >= 0 && yy < h && xx >= 0 && xx < w)
            o = *reinterpret_cast<const float2*>(head + (size_t)((long long)row + (long long)dy * (w + 2) + dx) * head_ld);
        const float4 wn = make_float4(mv[n].x * inv.x, mv[n].y * inv.y, mv[n].z * inv.z, mv[n].w * inv.w);
        amu.x += wn.x * o.x; amu.y += wn.y * o.x; amu.z += wn.z * o.x; amu.w += wn.w * o.x;
        av.x += wn.x * o.y; av.y += wn.y * o.y; av.z += wn.z * o.y; av.w += wn.w * o.y;
    }
    // activation_G on the upsampled v (DNET.py:57-59), in the reference's order
    av.x = (((av.x > 0.f) ? av.x : expm1f(av.x)) + 1.0f) + 1e-10f;
    av.y = (((av.y > 0.f) ? av.y : expm1f(av.y)) + 1.0f) + 1e-10f;
    av.z = (((av.z > 0.f) ? av.z : expm1f(av.z)) + 1.0f) + 1e-10f;
    av.w = (((av.w > 0.f) ? av.w : expm1f(av.w)) + 1.0f) + 1e-10f;
    const size_t W4 = (size_t)w * 4, plane = (size_t)h * 4 * W4;
    float* o0 = out + (size_t)b * 2 * plane + ((size_t)y * 4 + i) * W4 + (size_t)x * 4;
    *reinterpret_cast<float4*>(o0) = amu;
    *reinterpret_cast<float4*>(o0 + plane) = av;
}

}  // namespace

hipError_t launch_dnet_gauss_head(const float* in, int in_ld, int N, int h, int w, int pad, float* out, hipStream_t s) {
    const long long n = (long long)N * h * w;
    hipLaunchKernelGGL(dnet_gauss_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, in_ld, N, h, w, pad, out);
    return hipGetLastError();
}

hipError_t launch_dnet_upsample_gauss(const float* head, int head_ld, const float* mask, int mask_ld, int N, int h, int w, float* out,
                                      hipStream_t s) {
    const size_t n = (size_t)N * h * w * 4;
    hipLaunchKernelGGL(dnet_upsample_gauss_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, head, head_ld, mask, mask_ld,
                       N, h, w, out);
    return hipGetLastError();
}

}  // namespace magnet
