// dnet_kernels.hip — the part of MaGNet's D-Net decoder (DenseDepth_BN at downsample ratio 4, reference
// models/submodules/D_dense_depth.py:104-195, models/DNET.py:62-67) that is not a matrix-core convolution.
// The convolutions (conv2, up1..up3 with folded BatchNorm + LeakyReLU, the depth head) run on conv_mfma_kernel
// (magnet_conv_mfma_ex); the bilinear upsampling and the skip concatenation on the F-Net's kernels
// (magnet_upsample_bilinear_cl, magnet_pack_split).  What is left is the Gaussian activation behind the depth head.
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

}  // namespace

hipError_t launch_dnet_gauss_head(const float* in, int in_ld, int N, int h, int w, int pad, float* out, hipStream_t s) {
    const long long n = (long long)N * h * w;
    hipLaunchKernelGGL(dnet_gauss_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, in_ld, N, h, w, pad, out);
    return hipGetLastError();
}

}  // namespace magnet
