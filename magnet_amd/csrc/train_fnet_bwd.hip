// train_fnet_bwd.hip — the F-Net's backward in training mode (reference train_FNet.py:69-119: loss.backward() through the PSMNet of
// models/submodules/F_psmnet.py).  The input gradients of the convolutions run on conv_mfma.hip with flipped, transposed weight packs
// and the weight gradients on magnet_wgrad(_ex) (train_bwd.hip); this file holds the rest:
//
//   bn_bwd       BatchNorm2d backward with batch statistics: fp64 two-stage sums of g' and g' xhat (fixed order, no atomics), then
//                dx = gamma invstd (g' - mean g' - xhat mean g' xhat) as split-bf16 planes with zero borders; g' = g masked by
//                the forward's ReLU, recomputed from the saved pre-BN activations with the apply's own arithmetic
//   bn_bwd_sync  the same over several ranks (nn.SyncBatchNorm): the rank's two sums for the caller's all-gather, then the gathered
//                sums added in rank order, divided by the global count, and the same dx
//   grad_pack    the feature gradient (NCHW fp32) into the bordered split-bf16 grid of the last 1x1 layer
//   d2s_bwd      backward of the space-to-depth rearrangement (a gather)
//   spp_up_bwd   backward of the align_corners bilinear upsampling: per pooled cell, its weighted window gathered in a fixed order
//   spp_pool_bwd the skip connection's gradient: the concat slice plus the four average-pool backwards
//   stem_wgrad   firstconv.0's weight gradient (K = 27) from the fp32 image
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"

namespace magnet {

namespace {

constexpr int BB = MAGNET_BN_BLOCKS;

__device__ __forceinline__ uint16_t tb_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

__device__ __forceinline__ void tb_split(float v, uint16_t& h, uint16_t& l) {
    h = tb_bf16(v);
    l = tb_bf16(v - __uint_as_float((uint32_t)h << 16));
}

__device__ __forceinline__ float tb_join(const uint16_t* hi, const uint16_t* lo, size_t i) {
    return __uint_as_float((uint32_t)hi[i] << 16) + __uint_as_float((uint32_t)lo[i] << 16);
}

__device__ __forceinline__ long long tb_row(long long p, int h, int w, int hp, int wp, int pad) {
    const long long hw = (long long)h * w;
    const long long n = p / hw;
    const int r = (int)(p - n * hw);
    const int y = r / w, x = r - y * w;
    return (n * hp + y + pad) * wp + x + pad;
}

// g' and xhat at (row, c), exactly as bn_apply_kernel computed the forward's pre-ReLU value
__device__ __forceinline__ void tb_gx(const MagnetBnBwdArgs& a, long long row, int c, float& gp, float& xh) {
    const float x = a.x[row * a.x_ld + c];
    const float g = a.g[row * a.g_ld + c];
    xh = (x - a.mean[c]) * a.invstd[c];
    gp = g;
    if (a.relu) {
        float t = (x - a.mean[c]) * a.invstd[c] * a.gamma[c] + a.beta[c];
        t = t + 0.f;
        gp = t > 0.f ? g : 0.f;
    }
}

}  // namespace

// ---- BN backward, stage 1: workgroup b, positions [b P / BB, (b+1) P / BB); thread (slice, channel), 256 / C' slices ----
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const MagnetBnBwdArgs a) {
    __shared__ double red[2][256];
    const int h = a.hp - 2 * a.pad, w = a.wp - 2 * a.pad;
    const long long P = (long long)a.N * h * w;
    const long long p0 = P * blockIdx.x / BB, p1 = P * (blockIdx.x + 1) / BB;
    for (int c0 = 0; c0 < a.C; c0 += 256) {
        const int cw = a.C - c0 < 256 ? a.C - c0 : 256;           // channels of this pass
        const int nsl = 256 / cw;
        const int c = c0 + (int)threadIdx.x % cw, sl = (int)threadIdx.x / cw;
        double s1 = 0.0, s2 = 0.0;
        if (sl < nsl)
            for (long long p = p0 + sl; p < p1; p += nsl) {
                float gp, xh;
                tb_gx(a, tb_row(p, h, w, a.hp, a.wp, a.pad), c, gp, xh);
                s1 += (double)gp;
                s2 += (double)gp * (double)xh;
            }
        __syncthreads();
        red[0][threadIdx.x] = s1;
        red[1][threadIdx.x] = s2;
        __syncthreads();
        if ((int)threadIdx.x < cw) {
            double t1 = 0.0, t2 = 0.0;
            for (int i = 0; i < nsl; ++i) { t1 += red[0][i * cw + threadIdx.x]; t2 += red[1][i * cw + threadIdx.x]; }
            a.work[((size_t)blockIdx.x * a.C + c0 + threadIdx.x) * 2 + 0] = t1;
            a.work[((size_t)blockIdx.x * a.C + c0 + threadIdx.x) * 2 + 1] = t2;
        }
    }
}

// ---- stage 2: fixed-order sum over the workgroups; dgamma, dbeta, and the two means for the apply (after the partials) ----
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const MagnetBnBwdArgs a) {
    const int h = a.hp - 2 * a.pad, w = a.wp - 2 * a.pad;
    const double n = (double)((long long)a.N * h * w);
    double* m = a.work + (size_t)BB * a.C * 2;
    for (int c = threadIdx.x; c < a.C; c += 256) {
        double t1 = 0.0, t2 = 0.0;
        for (int b = 0; b < BB; ++b) { t1 += a.work[((size_t)b * a.C + c) * 2]; t2 += a.work[((size_t)b * a.C + c) * 2 + 1]; }
        a.dbeta[c] = (float)t1;
        a.dgamma[c] = (float)t2;
        m[2 * c] = t1 / n;
        m[2 * c + 1] = t2 / n;
    }
}

// ---- synchronised backward, local stage 2: this rank's sums of g' and g' xhat (xhat from the global mean / invstd) as
// ---- sums[(2, C)] in fp64; dgamma / dbeta are the local sums, as torch.nn.SyncBatchNorm leaves them to DDP's averaging ----
__global__ __launch_bounds__(256) void bn_bwd_sums_final_kernel(const MagnetBnBwdArgs a, double* __restrict__ sums) {
    for (int c = threadIdx.x; c < a.C; c += 256) {
        double t1 = 0.0, t2 = 0.0;
        for (int b = 0; b < BB; ++b) { t1 += a.work[((size_t)b * a.C + c) * 2]; t2 += a.work[((size_t)b * a.C + c) * 2 + 1]; }
        a.dbeta[c] = (float)t1;
        a.dgamma[c] = (float)t2;
        sums[c] = t1;
        sums[a.C + c] = t2;
    }
}

// ---- synchronised backward, after the all-gather: sums (world, 2, C) added in rank order and divided by the global count on the
// ---- device: the two means bn_bwd_apply_kernel reads ----
__global__ __launch_bounds__(256) void bn_bwd_sync_means_kernel(const MagnetBnBwdArgs a, const double* __restrict__ sums, int world,
                                                                const double* __restrict__ n_tot) {
    const double n = n_tot[0];
    double* m = a.work + (size_t)BB * a.C * 2;
    for (int c = threadIdx.x; c < a.C; c += 256) {
        double t1 = 0.0, t2 = 0.0;
        for (int r = 0; r < world; ++r) { t1 += sums[((size_t)r * 2) * a.C + c]; t2 += sums[((size_t)r * 2 + 1) * a.C + c]; }
        m[2 * c] = t1 / n;
        m[2 * c + 1] = t2 / n;
    }
}

// ---- stage 3: one thread per (grid row, channel) ----
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const MagnetBnBwdArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rows = (long long)a.N * a.hp * a.wp;
    if (idx >= rows * a.C) return;
    const int c = (int)(idx % a.C);
    const long long row = idx / a.C;
    const int rem = (int)(row % ((long long)a.hp * a.wp));
    const int y = rem / a.wp, x = rem - y * a.wp;
    const bool interior = y >= a.pad && y < a.hp - a.pad && x >= a.pad && x < a.wp - a.pad;
    float v = 0.f;
    if (interior) {
        const double* m = a.work + (size_t)BB * a.C * 2;
        float gp, xh;
        tb_gx(a, row, c, gp, xh);
        v = (float)((double)a.gamma[c] * (double)a.invstd[c] * ((double)gp - m[2 * c] - (double)xh * m[2 * c + 1]));
    }
    uint16_t hh, ll;
    tb_split(v, hh, ll);
    ((uint16_t*)a.dx_hi)[row * a.dx_ld + c] = hh;
    ((uint16_t*)a.dx_lo)[row * a.dx_ld + c] = ll;
}

// ---- feature gradient NCHW fp32 -> bordered split grid, channels [C, ld) zero ----
__global__ __launch_bounds__(256) void grad_pack_kernel(const float* __restrict__ in, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo,
                                                        int N, int C, int h, int w, int pad, int ld) {
    const int hp = h + 2 * pad, wp = w + 2 * pad;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * hp * wp * ld) return;
    const int c = (int)(idx % ld);
    const long long row = idx / ld;
    const int rem = (int)(row % ((long long)hp * wp));
    const int n = (int)(row / ((long long)hp * wp));
    const int y = rem / wp - pad, x = rem % wp - pad;
    float v = 0.f;
    if (c < C && y >= 0 && y < h && x >= 0 && x < w) v = in[(((size_t)n * C + c) * h + y) * w + x];
    uint16_t a, b;
    tb_split(v, a, b);
    hi[idx] = a;
    lo[idx] = b;
}

// ---- space-to-depth backward: out[n, y, x, c] = in[n, y/2, x/2, ((y%2)*2 + x%2) C + c] ----
__global__ __launch_bounds__(256) void d2s_bwd_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int C, int H2, int W2,
                                                      int H4, int W4, int ipad) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * H2 * W2 * C) return;
    const int c = (int)(idx % C);
    const long long pix = idx / C;
    const int x = (int)(pix % W2), y = (int)((pix / W2) % H2), n = (int)(pix / ((long long)W2 * H2));
    const size_t irow = ((size_t)n * (H4 + 2 * ipad) + (y / 2 + ipad)) * (W4 + 2 * ipad) + (x / 2 + ipad);
    const size_t orow = ((size_t)n * (H2 + 2) + (y + 1)) * (W2 + 2) + (x + 1);
    out[orow * C + c] = in[irow * 4 * C + ((y & 1) * 2 + (x & 1)) * C + c];
}

// ---- bilinear (align_corners) backward: workgroup = one pooled cell; thread (row slice of 8, channel of 32); the 1-D weights of
// ---- the cell along y and x are recomputed with the forward's arithmetic; slices summed in order ----
__device__ __forceinline__ float up_w(int o, int cell, int in_n, int out_n) {
    const float s = (out_n > 1) ? (float)(in_n - 1) / (float)(out_n - 1) : 0.f;
    const float f = s * (float)o;
    const int i0 = (int)f;
    const int i1 = i0 + ((i0 < in_n - 1) ? 1 : 0);
    const float l1 = f - (float)i0, l0 = 1.0f - l1;
    return (i0 == cell ? l0 : 0.f) + (i1 == cell ? l1 : 0.f);
}

__global__ __launch_bounds__(256) void spp_up_bwd_kernel(const MagnetSppBwdArgs a) {
    __shared__ float red[8][32];
    const int cell = blockIdx.x;
    const int px = cell % a.pw, py = (cell / a.pw) % a.ph, n = cell / (a.pw * a.ph);
    const int c = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int hp = a.h + 2 * a.pad, wp = a.w + 2 * a.pad;
    // output rows / columns whose weight on this cell can be nonzero: src in (cell - 1, cell + 1)
    const float sy = (a.h > 1) ? (float)(a.ph - 1) / (float)(a.h - 1) : 0.f, sx = (a.w > 1) ? (float)(a.pw - 1) / (float)(a.w - 1) : 0.f;
    int y0 = 0, y1 = a.h, x0 = 0, x1 = a.w;
    if (sy > 0.f) { y0 = (int)((float)(py - 1) / sy) - 1; y1 = (int)((float)(py + 1) / sy) + 2; }
    if (sx > 0.f) { x0 = (int)((float)(px - 1) / sx) - 1; x1 = (int)((float)(px + 1) / sx) + 2; }
    y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0; y1 = y1 > a.h ? a.h : y1; x1 = x1 > a.w ? a.w : x1;
    float s = 0.f;
    for (int y = y0 + sl; y < y1; y += 8) {
        const float wy = up_w(y, py, a.ph, a.h);
        if (wy == 0.f) continue;
        const float* gr = a.g + ((size_t)(n * hp + y + a.pad) * wp + a.pad) * a.g_ld + a.c_off + c;
        float r = 0.f;
        for (int x = x0; x < x1; ++x) {
            const float wx = up_w(x, px, a.pw, a.w);
            r += wx * gr[(size_t)x * a.g_ld];
        }
        s += wy * r;
    }
    red[sl][c] = s;
    __syncthreads();
    if (sl == 0) {
        float t = 0.f;
        for (int i = 0; i < 8; ++i) t += red[i][c];
        a.dq[(size_t)cell * 32 + c] = t;
    }
}

__global__ __launch_bounds__(256) void spp_pool_bwd_kernel(const MagnetSppBwdArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.N * a.h * a.w * 128) return;
    const int c = (int)(idx & 127);
    const long long pix = idx >> 7;
    const int x = (int)(pix % a.w), y = (int)((pix / a.w) % a.h), n = (int)(pix / ((long long)a.w * a.h));
    const size_t row = ((size_t)n * (a.h + 2 * a.pad) + (y + a.pad)) * (a.w + 2 * a.pad) + (x + a.pad);
    float v = a.g[row * a.g_ld + a.c_off + c];
    const int ks[4] = {64, 32, 16, 8};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int k = ks[b], ph = a.h / k, pw = a.w / k;
        if (y < ph * k && x < pw * k) v += a.dpool[b][((size_t)(n * ph + y / k) * pw + x / k) * 128 + c] / (float)(k * k);
    }
    a.out[row * a.out_ld + c] = v;
}

// ---- stem wgrad: stage 1, workgroup b sums positions [b P / BB, (b+1) P / BB) for all 864 weights (thread t: t, t+256, ...) ----
__global__ __launch_bounds__(256) void stem_wgrad_partial_kernel(const float* __restrict__ img, const uint16_t* __restrict__ dz_hi,
                                                                 const uint16_t* __restrict__ dz_lo, double* __restrict__ work,
                                                                 int N, int H, int W, int H2, int W2) {
    const long long P = (long long)N * H2 * W2;
    const long long p0 = P * blockIdx.x / BB, p1 = P * (blockIdx.x + 1) / BB;
    for (int o = threadIdx.x; o < 864; o += 256) {
        const int co = o / 27, k = o % 27, ci = k / 9, dy = (k % 9) / 3, dx = k % 3;
        float s = 0.f;
        for (long long p = p0; p < p1; ++p) {
            const int x = (int)(p % W2), y = (int)((p / W2) % H2), n = (int)(p / ((long long)W2 * H2));
            const int iy = 2 * y + dy - 1, ix = 2 * x + dx - 1;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const size_t row = ((size_t)n * (H2 + 2) + (y + 1)) * (W2 + 2) + (x + 1);
            s += tb_join(dz_hi, dz_lo, row * 32 + co) * img[(((size_t)n * 3 + ci) * H + iy) * W + ix];
        }
        work[(size_t)blockIdx.x * 864 + o] = (double)s;
    }
}

__global__ __launch_bounds__(256) void stem_wgrad_final_kernel(const double* __restrict__ work, float* __restrict__ grad_w) {
    for (int o = threadIdx.x; o < 864; o += 256) {
        double t = 0.0;
        for (int b = 0; b < BB; ++b) t += work[(size_t)b * 864 + o];
        grad_w[o] = (float)t;                                       // (32, 3, 3, 3): o = co * 27 + ci * 9 + dy * 3 + dx
    }
}

hipError_t launch_bn_train_backward(const MagnetBnBwdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(BB), dim3(256), 0, s, a);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(1), dim3(256), 0, s, a);
    const long long n = (long long)a.N * a.hp * a.wp * a.C;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bn_sync_backward_sums(const MagnetBnBwdArgs& a, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(BB), dim3(256), 0, s, a);
    hipLaunchKernelGGL(bn_bwd_sums_final_kernel, dim3(1), dim3(256), 0, s, a, sums);
    return hipGetLastError();
}

hipError_t launch_bn_sync_backward_apply(const MagnetBnBwdArgs& a, const double* sums, int world, const double* n_tot, hipStream_t s) {
    hipLaunchKernelGGL(bn_bwd_sync_means_kernel, dim3(1), dim3(256), 0, s, a, sums, world, n_tot);
    const long long n = (long long)a.N * a.hp * a.wp * a.C;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fnet_grad_pack(const float* in, uint16_t* hi, uint16_t* lo, int N, int C, int h, int w, int pad, int ld, hipStream_t s) {
    const long long n = (long long)N * (h + 2 * pad) * (w + 2 * pad) * ld;
    hipLaunchKernelGGL(grad_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, hi, lo, N, C, h, w, pad, ld);
    return hipGetLastError();
}

hipError_t launch_fnet_d2s_backward(const float* in, float* out, int N, int C, int H2, int W2, int ipad, hipStream_t s) {
    const int H4 = (H2 - 1) / 2 + 1, W4 = (W2 - 1) / 2 + 1;
    const long long n = (long long)N * H2 * W2 * C;
    hipLaunchKernelGGL(d2s_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, N, C, H2, W2, H4, W4, ipad);
    return hipGetLastError();
}

hipError_t launch_spp_upsample_backward(const MagnetSppBwdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(spp_up_bwd_kernel, dim3((unsigned)(a.N * a.ph * a.pw)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_spp_pool_backward(const MagnetSppBwdArgs& a, hipStream_t s) {
    const long long n = (long long)a.N * a.h * a.w * 128;
    hipLaunchKernelGGL(spp_pool_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fnet_stem_wgrad(const float* img, const uint16_t* dz_hi, const uint16_t* dz_lo, float* grad_w, double* work, int N, int H,
                                  int W, hipStream_t s) {
    const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(stem_wgrad_partial_kernel, dim3(BB), dim3(256), 0, s, img, dz_hi, dz_lo, work, N, H, W, H2, W2);
    hipLaunchKernelGGL(stem_wgrad_final_kernel, dim3(1), dim3(256), 0, s, work, grad_w);
    return hipGetLastError();
}

}  // namespace magnet
