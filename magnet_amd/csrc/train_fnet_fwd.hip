// train_fnet_fwd.hip — the F-Net's forward in training mode (reference train_FNet.py:69-119 with model.train(): every
// BatchNorm2d of models/submodules/F_psmnet.py normalises with the statistics of the batch and updates its running statistics).
// The convolutions are the inference kernels run without BatchNorm folding (conv_mfma.hip, fp32 pre-BN output); this file holds
//
//   stem_raw    firstconv.0 (3 -> 32, 3x3 stride 2) on the NCHW fp32 image without BN / ReLU: fp32 into the zero-bordered grid
//   bn_stats    per-channel batch mean and biased variance over the interior positions of every image: a fixed-order two-stage
//               reduction in fp64 (MAGNET_BN_BLOCKS workgroups over the positions -> partial sums -> one fixed-order final sum,
//               no atomics), shifted by the channel's first value so that the variance does not cancel; the final stage writes
//               mean, 1/sqrt(var + eps) and the running-statistics update on the device
//   bn_sync     the same statistics over several ranks (nn.SyncBatchNorm): stage 1 as above, a final stage that writes the rank's
//               (n, mean, M2) record instead, and, after the caller's all-gather, a merge of the records in rank order
//   bn_apply    y = (x - mean) * invstd * gamma + beta, + an optional split-bf16 residual, optional ReLU, written as split-bf16
//               planes (border rows zeroed; the output may be a channel slice of a wider buffer) or as fp32
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"

namespace magnet {

constexpr int BN_BLOCKS = MAGNET_BN_BLOCKS;

namespace {

__device__ __forceinline__ uint16_t tf_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// interior position p in [0, N*h*w) -> row of the bordered grid
__device__ __forceinline__ long long tf_row(long long p, int h, int w, int hp, int wp, int pad) {
    const long long hw = (long long)h * w;
    const long long n = p / hw;
    const int r = (int)(p - n * hw);
    const int y = r / w, x = r - y * w;
    return (n * hp + y + pad) * wp + x + pad;
}

}  // namespace

// ---- stem without BN: out[(n, y+1, x+1)][co] = sum_{ci,dy,dx} W[co][ci][dy][dx] * img[n, ci, 2y+dy-1, 2x+dx-1] (fp32, 32 ch) ----
__global__ __launch_bounds__(256) void fnet_stem_raw_kernel(const float* __restrict__ img, const float* __restrict__ wgt,
                                                            float* __restrict__ out, int N, int H, int W, int H2, int W2) {
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
                const int iy = 2 * y + dy - 1, ix = 2 * x + dx - 1;
                const bool ok = (iy >= 0) && (iy < H) && (ix >= 0) && (ix < W);
                in[ci * 9 + dy * 3 + dx] = ok ? img[(((size_t)n * 3 + ci) * H + iy) * W + ix] : 0.f;
            }
    float* o = out + (((size_t)n * (H2 + 2) + (y + 1)) * (W2 + 2) + (x + 1)) * 32;
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = c4 * 4 + i;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 27; ++k) acc = __builtin_fmaf(wgt[co * 27 + k], in[k], acc);
            v[i] = acc;
        }
        *reinterpret_cast<float4*>(o + c4 * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ---- BN statistics, stage 1: workgroup b sums the positions [b P / BN_BLOCKS, (b+1) P / BN_BLOCKS) of all C channels: thread
// ---- (slice, 8-channel chunk), C / 8 threads per position, 256 / (C / 8) position slices interleaved; then the slices in order ----
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const MagnetBnTrainArgs a) {
    __shared__ double red[2][2048];
    const int h = a.hp - 2 * a.pad, w = a.wp - 2 * a.pad;
    const long long P = (long long)a.N * h * w;
    const int cpr = a.C / 8, nsl = 256 / cpr;
    const int ch = threadIdx.x % cpr, sl = threadIdx.x / cpr;
    const long long p0 = P * blockIdx.x / BN_BLOCKS, p1 = P * (blockIdx.x + 1) / BN_BLOCKS;
    double s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s1[i] = 0.0; s2[i] = 0.0; }
    if (sl < nsl) {
        const float* xs = a.x + tf_row(0, h, w, a.hp, a.wp, a.pad) * a.x_ld + ch * 8;
        const float4 q0 = *reinterpret_cast<const float4*>(xs), q1 = *reinterpret_cast<const float4*>(xs + 4);
        const float sh[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        for (long long p = p0 + sl; p < p1; p += nsl) {
            const float* xp = a.x + tf_row(p, h, w, a.hp, a.wp, a.pad) * a.x_ld + ch * 8;
            const float4 v0 = *reinterpret_cast<const float4*>(xp), v1 = *reinterpret_cast<const float4*>(xp + 4);
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double d = (double)v[i] - (double)sh[i];
                s1[i] += d;
                s2[i] += d * d;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) { red[0][sl * a.C + ch * 8 + i] = s1[i]; red[1][sl * a.C + ch * 8 + i] = s2[i]; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < a.C; c += 256) {
        double t1 = 0.0, t2 = 0.0;
        for (int i = 0; i < nsl; ++i) { t1 += red[0][i * a.C + c]; t2 += red[1][i * a.C + c]; }
        a.work[((size_t)blockIdx.x * a.C + c) * 2 + 0] = t1;
        a.work[((size_t)blockIdx.x * a.C + c) * 2 + 1] = t2;
    }
}

// ---- stage 2: one workgroup; thread c sums the BN_BLOCKS partials in order, then mean / invstd and the running update
// ---- (nn.BatchNorm2d: running = (1 - m) running + m stat, the variance unbiased; momentum < 0: m = 1 / (tracked + 1)) ----
__global__ __launch_bounds__(512) void bn_stats_final_kernel(const MagnetBnTrainArgs a) {
    const int h = a.hp - 2 * a.pad, w = a.wp - 2 * a.pad;
    const long long P = (long long)a.N * h * w;
    const double n = (double)P;
    double m = a.momentum;
    if (m < 0.0) m = 1.0 / (double)((a.num_batches_tracked ? a.num_batches_tracked[0] : 0) + 1);
    __syncthreads();                                    // every thread has read num_batches_tracked before it is updated
    for (int c = threadIdx.x; c < a.C; c += 512) {
        double t1 = 0.0, t2 = 0.0;
        for (int b = 0; b < BN_BLOCKS; ++b) { t1 += a.work[((size_t)b * a.C + c) * 2]; t2 += a.work[((size_t)b * a.C + c) * 2 + 1]; }
        const double shift = (double)a.x[tf_row(0, h, w, a.hp, a.wp, a.pad) * a.x_ld + c];
        const double dm = t1 / n;
        double var = t2 / n - dm * dm;
        var = var > 0.0 ? var : 0.0;
        const double mean = shift + dm;
        a.mean[c] = (float)mean;
        a.invstd[c] = (float)(1.0 / sqrt(var + a.eps));
        if (a.running_mean) a.running_mean[c] = (float)((1.0 - m) * (double)a.running_mean[c] + m * mean);
        if (a.running_var) a.running_var[c] = (float)((1.0 - m) * (double)a.running_var[c] + m * var * n / (n - 1.0));
    }
    if (threadIdx.x == 0 && a.num_batches_tracked) a.num_batches_tracked[0] += 1;
}

// ---- synchronised statistics, local stage 2 (after bn_stats_partial_kernel): thread c sums the BN_BLOCKS partials in order and
// ---- writes this rank's record (n, mean, M2 = sum (x - mean)^2) as rec[(3, C)].  Unlike the shifted sums, whose shift is the
// ---- shard's own first value, the record means the same on every rank.  mean / invstd / the running statistics: untouched ----
__global__ __launch_bounds__(512) void bn_moments_final_kernel(const MagnetBnTrainArgs a, double* __restrict__ rec) {
    const int h = a.hp - 2 * a.pad, w = a.wp - 2 * a.pad;
    const double n = (double)((long long)a.N * h * w);
    for (int c = threadIdx.x; c < a.C; c += 512) {
        double t1 = 0.0, t2 = 0.0;
        for (int b = 0; b < BN_BLOCKS; ++b) { t1 += a.work[((size_t)b * a.C + c) * 2]; t2 += a.work[((size_t)b * a.C + c) * 2 + 1]; }
        const double shift = (double)a.x[tf_row(0, h, w, a.hp, a.wp, a.pad) * a.x_ld + c];
        const double m2 = t2 - t1 * (t1 / n);
        rec[c] = n;
        rec[a.C + c] = shift + t1 / n;
        rec[2 * a.C + c] = m2 > 0.0 ? m2 : 0.0;
    }
}

// ---- synchronised statistics, merge: recs (world, 3, C), the ranks' records in rank order (the all-gather's output, the same
// ---- bytes on every rank).  Thread c: n_tot = sum n_r, mean = sum n_r mean_r / n_tot, M2 = sum (M2_r + n_r (mean_r - mean)^2), every
// ---- sum in rank order in fp64; then mean / invstd / n_tot and the running update of bn_stats_final_kernel with the global count ----
__global__ __launch_bounds__(512) void bn_sync_merge_kernel(const MagnetBnTrainArgs a, const double* __restrict__ recs, int world,
                                                            double* __restrict__ n_tot) {
    double m = a.momentum;
    if (m < 0.0) m = 1.0 / (double)((a.num_batches_tracked ? a.num_batches_tracked[0] : 0) + 1);
    __syncthreads();                                    // every thread has read num_batches_tracked before it is updated
    for (int c = threadIdx.x; c < a.C; c += 512) {
        double n = 0.0, s = 0.0;
        for (int r = 0; r < world; ++r) {
            const double* q = recs + (size_t)r * 3 * a.C;
            n += q[c];
            s += q[c] * q[a.C + c];
        }
        const double mean = s / n;
        double M2 = 0.0;
        for (int r = 0; r < world; ++r) {
            const double* q = recs + (size_t)r * 3 * a.C;
            const double d = q[a.C + c] - mean;
            M2 += q[2 * a.C + c] + q[c] * (d * d);
        }
        const double var = M2 / n;
        a.mean[c] = (float)mean;
        a.invstd[c] = (float)(1.0 / sqrt(var + a.eps));
        if (a.running_mean) a.running_mean[c] = (float)((1.0 - m) * (double)a.running_mean[c] + m * mean);
        if (a.running_var) a.running_var[c] = (float)((1.0 - m) * (double)a.running_var[c] + m * var * n / (n - 1.0));
        if (c == 0) n_tot[0] = n;
    }
    if (threadIdx.x == 0 && a.num_batches_tracked) a.num_batches_tracked[0] += 1;
}

// ---- apply: one thread per (grid row, 8 channels); rows outside the interior write zeros (split output) ----
__global__ __launch_bounds__(256) void bn_apply_kernel(const MagnetBnTrainArgs a) {
    const int cpr = a.C / 8;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rows = (long long)a.N * a.hp * a.wp;
    if (idx >= rows * cpr) return;
    const int c0 = (int)(idx % cpr) * 8;
    const long long row = idx / cpr;
    const int rem = (int)(row % ((long long)a.hp * a.wp));
    const int y = rem / a.wp, x = rem - y * a.wp;
    const bool interior = y >= a.pad && y < a.hp - a.pad && x >= a.pad && x < a.wp - a.pad;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (interior) {
        const float4 x0 = *reinterpret_cast<const float4*>(a.x + row * a.x_ld + c0);
        const float4 x1 = *reinterpret_cast<const float4*>(a.x + row * a.x_ld + c0 + 4);
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a.res_hi) {
            const uint4 rh = *reinterpret_cast<const uint4*>((const uint16_t*)a.res_hi + row * a.res_ld + c0);
            const uint4 rl = *reinterpret_cast<const uint4*>((const uint16_t*)a.res_lo + row * a.res_ld + c0);
            const uint32_t hw_[4] = {rh.x, rh.y, rh.z, rh.w}, lw_[4] = {rl.x, rl.y, rl.z, rl.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rv[2 * i]     = __uint_as_float(hw_[i] << 16) + __uint_as_float(lw_[i] << 16);
                rv[2 * i + 1] = __uint_as_float(hw_[i] & 0xffff0000u) + __uint_as_float(lw_[i] & 0xffff0000u);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = c0 + i;
            float t = (xv[i] - a.mean[c]) * a.invstd[c] * a.gamma[c] + a.beta[c];
            t = t + rv[i];
            v[i] = (a.relu && t < 0.f) ? 0.f : t;
        }
    }
    if (a.out_f32) {
        if (!interior) return;
        float* o = a.out_f32 + row * a.out_ld + c0;
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        return;
    }
    uint32_t hh[4], ll[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint16_t h0 = tf_bf16(v[2 * i]), h1 = tf_bf16(v[2 * i + 1]);
        const uint16_t l0 = tf_bf16(v[2 * i] - __uint_as_float((uint32_t)h0 << 16));
        const uint16_t l1 = tf_bf16(v[2 * i + 1] - __uint_as_float((uint32_t)h1 << 16));
        hh[i] = (uint32_t)h0 | ((uint32_t)h1 << 16);
        ll[i] = (uint32_t)l0 | ((uint32_t)l1 << 16);
    }
    *reinterpret_cast<uint4*>((uint16_t*)a.out_hi + row * a.out_ld + c0) = make_uint4(hh[0], hh[1], hh[2], hh[3]);
    *reinterpret_cast<uint4*>((uint16_t*)a.out_lo + row * a.out_ld + c0) = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}

hipError_t launch_fnet_stem_raw(const float* img, const float* wgt, float* out, int N, int H, int W, hipStream_t s) {
    const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1;
    const long long n = (long long)N * H2 * W2;
    hipLaunchKernelGGL(fnet_stem_raw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, img, wgt, out, N, H, W, H2, W2);
    return hipGetLastError();
}

hipError_t launch_bn_train_stats(const MagnetBnTrainArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(BN_BLOCKS), dim3(256), 0, s, a);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(1), dim3(512), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bn_sync_moments(const MagnetBnTrainArgs& a, double* rec, hipStream_t s) {
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(BN_BLOCKS), dim3(256), 0, s, a);
    hipLaunchKernelGGL(bn_moments_final_kernel, dim3(1), dim3(512), 0, s, a, rec);
    return hipGetLastError();
}

hipError_t launch_bn_sync_merge(const MagnetBnTrainArgs& a, const double* recs, int world, double* n_tot, hipStream_t s) {
    hipLaunchKernelGGL(bn_sync_merge_kernel, dim3(1), dim3(512), 0, s, a, recs, world, n_tot);
    return hipGetLastError();
}

hipError_t launch_bn_train_apply(const MagnetBnTrainArgs& a, hipStream_t s) {
    const long long n = (long long)a.N * a.hp * a.wp * (a.C / 8);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace magnet
