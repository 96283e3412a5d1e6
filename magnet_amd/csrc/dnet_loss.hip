// dnet_loss.hip — the tail of the stand-alone D-Net's training step behind the two head convolutions (reference
// models/submodules/D_dense_depth.py:86-100 upsample_depth_via_mask, models/DNET.py:56-60 activation_G, utils/losses.py:8-24 DnetLoss)
// from the raw head output depth (B, 2, h, w) [mu, v] and the 144 mask logits per coarse pixel (channel t*16 + i*4 + j, t = 3(dy+1) +
// (dx+1): unfold order), addressed through element strides.  Per fine pixel (4y+i, 4x+j):
//   w_t = softmax over the 9 taps;  mu = sum_t w_t depth[0](y+dy, x+dx),  vu likewise for channel 1 (zero outside the image, decided by
//   index);  var = (elu(vu) + 1) + 1e-10;  nll = (mu - gt)^2 / (2 var) + 0.5 log var;  loss = mean over the valid pixels.
//
//   dnl_forward_kernel   the upsampling in the operation order of dnet_upsample_gauss_kernel (max, expf(l - max), sum in ascending t,
//                        inv = 1 / den, w = e * inv, acc += w * o), so the optional pred output (B, 2, 4h, 4w) [mu, var] is that kernel's
//                        to the bit; count and NLL sum of the workgroup's valid pixels in fp64 -> one partial pair per workgroup.
//   dnl_final_kernel     the partial pairs summed in a fixed order, loss = sum / count (0 / 0 = NaN with no valid pixel).  No atomics:
//                        bit-identical from run to run.
//   dnl_backward_kernel  the softmax, mu, vu and var recomputed from the logits (nothing at full resolution is kept); with c =
//                        grad_loss / count (both read on the device), d = mu - gt:  g_mu = c d / var,  g_v = c (0.5 / var - d^2 / (2 var^2))
//                        elu'(vu) on valid pixels, 0 elsewhere;  G_t = g_mu depth[0](p + off_t) + g_v depth[1](p + off_t);
//                        grad_mask[t,i,j] = w_t (G_t - sum_u w_u G_u), every channel of every pixel written; and per (channel, tap) the
//                        sum over the 16 sub-pixels of w_t g_c -> work (B, 2, 9, h, w).  A wave with no valid pixel stores zeros
//                        without reading the logits.
//   dnl_gather_kernel    grad_depth[c](q) = sum_t work[c][t](q - off_t) in fixed tap order (sources outside the image give nothing),
//                        as upbwd_gather_kernel.
//   dnl_plain_*          the reference's own call on an already upsampled pred (B, 2, H, W) [mu, var]: the same NLL with var as it is;
//                        here the clamp var < 1e-10 -> 1e-10 (losses.py:19) does occur and leaves var without gradient.
//
// Mapping: workgroup = 64 consecutive coarse pixels (x fastest) x the 4 sub-rows i, one wave per sub-row: lane = coarse pixel, so
// every NCHW channel plane of the logits (and of their gradient) is read (written) as full 256-byte wave rows, and the 4 sub-columns
// j of a lane are one 16-byte access to gt / valid / pred.  A lane issues its 36 logit loads together; the sub-rows meet once in LDS (the
// fp64 partial sums of the forward, the 18 tap sums per pixel of the backward, added in the order i = 0..3).  Streaming, memory-bound:
// the forward reads the logits once (576 B per coarse pixel), the backward reads them once and writes their gradient once; expf,
// expm1f and logf are the accurate ones, as in the neighbouring kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"

namespace magnet {

namespace {

constexpr int PLAIN_BLOCKS = MAGNET_NLL_BLOCKS;

struct DnlP {
    const float* depth; const float* mask; const float* gt; const uint8_t* valid;
    float* pred; double* work; const double* sums; const float* grad_loss; float* gmask; float* part;
    long long sb, sc, sy, sx, gsb, gsc, gsy, gsx;
    long long npix;
    int h, w;
};

// losses.py:19-21 on one pixel.  In the fused form var = (elu + 1) + 1e-10 >= 1e-10 in fp32 (elu + 1 >= 0 and the sum rounds
// monotonically), so `clamped` cannot come out true there; the test stays for the plain form and to keep the two forms one expression.
__device__ __forceinline__ float dnl_clamp(float var, bool& clamped) {
    clamped = var < 1e-10f;
    return clamped ? 1e-10f : var;
}

__device__ __forceinline__ float dnl_nll(float d, float var) { return d * d / (2.f * var) + 0.5f * logf(var); }

__device__ __forceinline__ float dnl_gmu(float c, float d, float var) { return c * (d / var); }

__device__ __forceinline__ float dnl_gvar(float c, float d, float var) { return c * (0.5f / var - d * d / (2.f * var * var)); }

// softmax weights of the 4 sub-pixels j of sub-row i (l[t][j] in: logits, out: weights) and the convex combinations of the 3x3
// neighbourhood: dnet_upsample_gauss_kernel's arithmetic, operation for operation
__device__ __forceinline__ void dnl_upsample(float l[9][4], const float o0[9], const float o1[9], float mu[4], float vu[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float mx = -3.4e38f;
#pragma unroll
        for (int t = 0; t < 9; ++t) mx = fmaxf(mx, l[t][j]);
        float den = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) { l[t][j] = expf(l[t][j] - mx); den += l[t][j]; }
        const float inv = 1.0f / den;
        float am = 0.f, av = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            l[t][j] = l[t][j] * inv;
            am += l[t][j] * o0[t];
            av += l[t][j] * o1[t];
        }
        mu[j] = am; vu[j] = av;
    }
}

__device__ __forceinline__ float dnl_var(float vu) { return (((vu > 0.f) ? vu : expm1f(vu)) + 1.0f) + 1e-10f; }   // DNET.py:57-59

__device__ __forceinline__ void dnl_neighbours(const float* __restrict__ depth, long long b, int y, int x, int h, int w, float o0[9],
                                               float o1[9]) {
    const size_t hw = (size_t)h * w;
    const float* d0 = depth + (size_t)b * 2 * hw;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const size_t o = in ? (size_t)yy * w + xx : 0;
        const float a = d0[o], c = d0[hw + o];                  // always an address inside the image; the value counts only inside
        o0[t] = in ? a : 0.f;
        o1[t] = in ? c : 0.f;
    }
}

__global__ __launch_bounds__(256) void dnl_forward_kernel(const DnlP a) {
    __shared__ double red[2][256];
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * 64 + lane;
    double cnt = 0.0, sum = 0.0;
    if (q < a.npix) {
        const long long hw = (long long)a.h * a.w, b = q / hw;
        const int yx = (int)(q - b * hw), y = yx / a.w, x = yx - y * a.w;
        const float* mb = a.mask + b * a.sb + (long long)y * a.sy + (long long)x * a.sx;
        float l[9][4];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) l[t][j] = mb[(long long)(t * 16 + i * 4 + j) * a.sc];
        float o0[9], o1[9], mu[4], vu[4];
        dnl_neighbours(a.depth, b, y, x, a.h, a.w, o0, o1);
        const size_t W = (size_t)a.w * 4, HW = (size_t)a.h * 4 * W;
        const size_t fo = (size_t)b * HW + ((size_t)y * 4 + i) * W + (size_t)x * 4;
        const float4 g4 = *reinterpret_cast<const float4*>(a.gt + fo);
        const uint32_t v4 = *reinterpret_cast<const uint32_t*>(a.valid + fo);
        dnl_upsample(l, o0, o1, mu, vu);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
        float var[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            var[j] = dnl_var(vu[j]);
            if ((v4 >> (8 * j)) & 0xffu) {
                bool cl;
                const float vc = dnl_clamp(var[j], cl);
                cnt += 1.0;
                sum += (double)dnl_nll(mu[j] - g[j], vc);
            }
        }
        if (a.pred) {
            float* p0 = a.pred + (size_t)b * 2 * HW + (fo - (size_t)b * HW);
            *reinterpret_cast<float4*>(p0) = make_float4(mu[0], mu[1], mu[2], mu[3]);
            *reinterpret_cast<float4*>(p0 + HW) = make_float4(var[0], var[1], var[2], var[3]);
        }
    }
    red[0][threadIdx.x] = cnt;
    red[1][threadIdx.x] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            red[0][threadIdx.x] += red[0][threadIdx.x + st];
            red[1][threadIdx.x] += red[1][threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.work[(size_t)blockIdx.x * 2] = red[0][0];
        a.work[(size_t)blockIdx.x * 2 + 1] = red[1][0];
    }
}

// nparts (count, sum) pairs -> sums, loss.  Thread t adds the pairs t, t + 256, ... in ascending order, then a fixed tree.
__global__ __launch_bounds__(256) void dnl_final_kernel(const double* __restrict__ work, long long nparts, double* __restrict__ sums,
                                                        float* __restrict__ loss) {
    __shared__ double red[2][256];
    double cnt = 0.0, sum = 0.0;
    for (long long p = threadIdx.x; p < nparts; p += 256) {
        cnt += work[(size_t)p * 2];
        sum += work[(size_t)p * 2 + 1];
    }
    red[0][threadIdx.x] = cnt;
    red[1][threadIdx.x] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            red[0][threadIdx.x] += red[0][threadIdx.x + st];
            red[1][threadIdx.x] += red[1][threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[0] = red[0][0];
        sums[1] = red[1][0];
        *loss = (float)(red[1][0] / red[0][0]);             // no valid pixel: 0 / 0 = NaN, as torch.mean of an empty selection
    }
}

__global__ __launch_bounds__(256) void dnl_backward_kernel(const DnlP a) {
    __shared__ float ps[4][18][64];                          // per sub-row i: the tap sums (channel * 9 + tap) of the 64 pixels
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * 64 + lane;
    const long long hw = (long long)a.h * a.w;
    const bool in = q < a.npix;
    float acc0[9], acc1[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) { acc0[t] = 0.f; acc1[t] = 0.f; }
    long long b = 0;
    int y = 0, x = 0;
    uint32_t v4 = 0;
    size_t fo = 0;
    if (in) {
        b = q / hw;
        const int yx = (int)(q - b * hw);
        y = yx / a.w; x = yx - y * a.w;
        const size_t W = (size_t)a.w * 4;
        fo = (size_t)b * (size_t)a.h * 4 * W + ((size_t)y * 4 + i) * W + (size_t)x * 4;
        v4 = *reinterpret_cast<const uint32_t*>(a.valid + fo);
    }
    float* gb = a.gmask + b * a.gsb + (long long)y * a.gsy + (long long)x * a.gsx;
    if (__ballot(v4 != 0u) == 0) {                           // wave-uniform: no valid pixel under this wave, the logits are not read
        if (in) {
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) gb[(long long)(t * 16 + i * 4 + j) * a.gsc] = 0.f;
        }
    } else if (in) {
        const float* mb = a.mask + b * a.sb + (long long)y * a.sy + (long long)x * a.sx;
        float l[9][4];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) l[t][j] = mb[(long long)(t * 16 + i * 4 + j) * a.sc];
        float o0[9], o1[9], mu[4], vu[4];
        dnl_neighbours(a.depth, b, y, x, a.h, a.w, o0, o1);
        const float4 g4 = *reinterpret_cast<const float4*>(a.gt + fo);
        const float c = (float)((double)(*a.grad_loss) / a.sums[0]);
        dnl_upsample(l, o0, o1, mu, vu);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gm = 0.f, gv = 0.f;
            if ((v4 >> (8 * j)) & 0xffu) {
                bool cl;
                const float var = dnl_clamp(dnl_var(vu[j]), cl);
                const float d = mu[j] - g[j];
                gm = dnl_gmu(c, d, var);
                const float de = (vu[j] > 0.f) ? 1.0f : expf(vu[j]);             // d elu / d vu
                gv = cl ? 0.f : dnl_gvar(c, d, var) * de;
            }
            float G[9], S = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                G[t] = gm * o0[t] + gv * o1[t];
                S += l[t][j] * G[t];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                gb[(long long)(t * 16 + i * 4 + j) * a.gsc] = l[t][j] * (G[t] - S);
                acc0[t] += l[t][j] * gm;
                acc1[t] += l[t][j] * gv;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) { ps[i][t][lane] = acc0[t]; ps[i][9 + t][lane] = acc1[t]; }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 18 * 64; idx += 256) {
        const int ct = idx >> 6, ln = idx & 63;
        const long long qq = (long long)blockIdx.x * 64 + ln;
        if (qq >= a.npix) continue;
        const float s = ((ps[0][ct][ln] + ps[1][ct][ln]) + ps[2][ct][ln]) + ps[3][ct][ln];
        const long long bb = qq / hw;
        const int c = ct / 9, t = ct - c * 9;
        a.part[(size_t)((bb * 2 + c) * 9 + t) * (size_t)hw + (size_t)(qq - bb * hw)] = s;
    }
}

__global__ __launch_bounds__(256) void dnl_gather_kernel(const float* __restrict__ part, float* __restrict__ gdepth, long long nout,
                                                         int h, int w) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nout) return;
    const long long hw = (long long)h * w;
    const size_t img = (size_t)(q / hw);
    const int yx = (int)(q - (long long)img * hw), Y = yx / w, X = yx - Y * w;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int y = Y - (t / 3 - 1), x = X - (t % 3 - 1);
        if (y >= 0 && y < h && x >= 0 && x < w) s += part[(img * 9 + t) * (size_t)hw + (size_t)y * w + x];
    }
    gdepth[q] = s;
}

__global__ __launch_bounds__(256) void dnl_plain_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const uint8_t* __restrict__ valid, double* __restrict__ work,
                                                                long long npix, long long hw) {
    __shared__ double red[2][256];
    double cnt = 0.0, sum = 0.0;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long long)PLAIN_BLOCKS * 256) {
        if (!valid[q]) continue;
        const long long b = q / hw;
        const size_t o = (size_t)b * 2 * hw + (size_t)(q - b * hw);
        bool cl;
        const float var = dnl_clamp(pred[o + hw], cl);
        cnt += 1.0;
        sum += (double)dnl_nll(pred[o] - gt[q], var);
    }
    red[0][threadIdx.x] = cnt;
    red[1][threadIdx.x] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            red[0][threadIdx.x] += red[0][threadIdx.x + st];
            red[1][threadIdx.x] += red[1][threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        work[(size_t)blockIdx.x * 2] = red[0][0];
        work[(size_t)blockIdx.x * 2 + 1] = red[1][0];
    }
}

__global__ __launch_bounds__(256) void dnl_plain_backward_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const uint8_t* __restrict__ valid, const double* __restrict__ sums,
                                                                 const float* __restrict__ grad_loss, float* __restrict__ grad_pred,
                                                                 long long npix, long long hw) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= npix) return;
    const long long b = q / hw;
    const size_t o = (size_t)b * 2 * hw + (size_t)(q - b * hw);
    float gm = 0.f, gv = 0.f;
    if (valid[q]) {
        const float c = (float)((double)(*grad_loss) / sums[0]);
        bool cl;
        const float var = dnl_clamp(pred[o + hw], cl);
        const float d = pred[o] - gt[q];
        gm = dnl_gmu(c, d, var);
        gv = cl ? 0.f : dnl_gvar(c, d, var);
    }
    grad_pred[o] = gm;
    grad_pred[o + hw] = gv;
}

DnlP dnl_params(const MagnetDnetLossArgs& a) {
    DnlP p{};
    p.depth = a.depth; p.mask = a.mask; p.gt = a.gt; p.valid = a.valid; p.pred = a.pred; p.sums = a.sums; p.grad_loss = a.grad_loss;
    p.gmask = a.grad_mask;
    p.sb = a.mask_sb; p.sc = a.mask_sc; p.sy = a.mask_sy; p.sx = a.mask_sx;
    p.gsb = a.gm_sb; p.gsc = a.gm_sc; p.gsy = a.gm_sy; p.gsx = a.gm_sx;
    p.npix = (long long)a.B * a.h * a.w; p.h = a.h; p.w = a.w;
    return p;
}

}  // namespace

long long dnet_loss_workspace_bytes(const MagnetDnetLossArgs& a) {
    const long long npix = (long long)a.B * a.h * a.w;
    const long long fwd = (npix + 63) / 64 * 2 * (long long)sizeof(double), bwd = npix * 18 * (long long)sizeof(float);
    return fwd > bwd ? fwd : bwd;
}

hipError_t launch_dnet_loss_forward(const MagnetDnetLossArgs& a, hipStream_t s) {
    DnlP p = dnl_params(a);
    p.work = (double*)a.work;
    const long long nblk = (p.npix + 63) / 64;
    hipLaunchKernelGGL(dnl_forward_kernel, dim3((unsigned)nblk), dim3(256), 0, s, p);
    hipLaunchKernelGGL(dnl_final_kernel, dim3(1), dim3(256), 0, s, (const double*)a.work, nblk, a.sums, a.loss);
    return hipGetLastError();
}

hipError_t launch_dnet_loss_backward(const MagnetDnetLossArgs& a, hipStream_t s) {
    DnlP p = dnl_params(a);
    p.part = (float*)a.work;
    const long long nblk = (p.npix + 63) / 64, nout = p.npix * 2;
    hipLaunchKernelGGL(dnl_backward_kernel, dim3((unsigned)nblk), dim3(256), 0, s, p);
    hipLaunchKernelGGL(dnl_gather_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, (const float*)a.work, a.grad_depth, nout,
                       a.h, a.w);
    return hipGetLastError();
}

hipError_t launch_dnet_nll_forward(const MagnetDnetNllArgs& a, hipStream_t s) {
    const long long hw = (long long)a.H * a.W, npix = (long long)a.B * hw;
    hipLaunchKernelGGL(dnl_plain_partial_kernel, dim3(PLAIN_BLOCKS), dim3(256), 0, s, a.pred, a.gt, a.valid, a.work, npix, hw);
    hipLaunchKernelGGL(dnl_final_kernel, dim3(1), dim3(256), 0, s, (const double*)a.work, (long long)PLAIN_BLOCKS, a.sums, a.loss);
    return hipGetLastError();
}

hipError_t launch_dnet_nll_backward(const MagnetDnetNllArgs& a, hipStream_t s) {
    const long long hw = (long long)a.H * a.W, npix = (long long)a.B * hw;
    hipLaunchKernelGGL(dnl_plain_backward_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, a.pred, a.gt, a.valid, a.sums,
                       a.grad_loss, a.grad_pred, npix, hw);
    return hipGetLastError();
}

}  // namespace magnet
