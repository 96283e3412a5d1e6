// train_bwd.hip — the HIP training step of G-Net and the mask head (reference: train_MaGNet.py:87-98, models/MAGNET.py:15-27,
// 47-70,111-118, utils/losses.py:28-52).  Forward reuses the inference kernels (conv_mfma.hip layer by layer, the Gaussian update
// and the convex upsampling); this file holds the backward and the loss:
//
//   nll_*        Gaussian NLL of every iteration (MagnetLoss 'gaussian'): a deterministic two-stage reduction (fixed grid of
//                NLL_BLOCKS workgroups -> partial sums -> one fixed-order final sum, no atomics) and the per-pixel backward, which
//                reads dL/dloss on the device (GradScaler's scale never touches the host).
//   upbwd_*      convex-upsampling backward as two gathers: per (pixel, tap) partial sums of softmax * d up, then a fixed-order
//                9-neighbour gather for d depth; d mask (softmax backward) summed over the iterations, which share the mask.
//   dgrad_*      the 1x1 tail backward of a stack, one launch: dh3 = W4^T dout [h3>0], dh2 = W3^T dh3 [h2>0], dh1 = W2^T dh2 [h1>0]
//                on v_mfma_f32_16x16x32_bf16 with bf16x3 split operands (as conv_mfma.hip); the gradient tile stays in LDS
//                between the three products.  G-Net's form computes dout from d(mu, sigma) through the Gaussian update itself.
//   wgrad_*      dW[tap][o][c] = sum_rows dY[row][o] X[row + off(tap)][c] on the matrix cores: both operands are channel-last, so
//                the row (K) dimension is strided; tiles are staged row-major in LDS and fed to the MFMA with ds_read_b64_tr_b16.
//                Rows are split into fixed chunks (partial tiles), then a fixed-order reduction maps the sum into nn.Conv2d's
//                (Cout, Cin, kh, kw) layout: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"
#include "warp_math.hpp"

namespace magnet {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;

constexpr int NLL_BLOCKS = MAGNET_NLL_BLOCKS;
constexpr int NLL_MAX_ITER = MAGNET_NLL_MAX_ITER;
constexpr int WG_CHUNK = MAGNET_WGRAD_CHUNK;

// ---------------------------------------------------------------------------------------------------------------------
// Gaussian NLL (utils/losses.py:34-50)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float nll_var(float sigma, bool& clamped) {
    float var = sigma * sigma;
    clamped = var < 1e-10f;                       // losses.py: var[var < 1e-10] = 1e-10 (in place: no gradient there)
    return clamped ? 1e-10f : var;
}

__global__ __launch_bounds__(256) void nll_partial_kernel(const float* __restrict__ preds, const float* __restrict__ gt,
                                                          const uint8_t* __restrict__ mask, double* __restrict__ work,
                                                          int n_iter, int B, int hw) {
    __shared__ double red[256];
    double s[NLL_MAX_ITER + 1];
#pragma unroll
    for (int i = 0; i <= NLL_MAX_ITER; ++i) s[i] = 0.0;
    const long long npix = (long long)B * hw;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long long)NLL_BLOCKS * 256) {
        if (!mask[q]) continue;
        const int b = (int)(q / hw), yx = (int)(q - (long long)b * hw);
        const float g = gt[q];
        s[0] += 1.0;
#pragma unroll
        for (int i = 0; i < NLL_MAX_ITER; ++i) {
            if (i >= n_iter) break;
            const float* p = preds + ((size_t)(i * B + b) * 2) * hw + yx;
            const float mu = p[0], sigma = p[hw];
            bool cl;
            const float var = nll_var(sigma, cl);
            const float d = mu - g;
            s[1 + i] += (double)(d * d / (2.f * var) + 0.5f * logf(var));
        }
    }
    for (int i = 0; i <= n_iter; ++i) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j <= NLL_MAX_ITER; ++j) if (j == i) v = s[j];
        red[threadIdx.x] = v;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) work[(size_t)blockIdx.x * (n_iter + 1) + i] = red[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void nll_final_kernel(const double* __restrict__ work, double* __restrict__ sums, float* __restrict__ loss,
                                                       int n_iter, double gamma) {
    __shared__ double tot[NLL_MAX_ITER + 1];
    const int t = threadIdx.x;
    if (t <= n_iter) {
        double v = 0.0;
        for (int b = 0; b < NLL_BLOCKS; ++b) v += work[(size_t)b * (n_iter + 1) + t];     // fixed order
        tot[t] = v;
        sums[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        double l = 0.0;
        for (int i = 0; i < n_iter; ++i) l += pow(gamma, (double)(n_iter - 1 - i)) * (tot[1 + i] / tot[0]);
        *loss = (float)l;
    }
}

__global__ __launch_bounds__(256) void nll_backward_kernel(const float* __restrict__ preds, const float* __restrict__ gt,
                                                           const uint8_t* __restrict__ mask, const double* __restrict__ sums,
                                                           const float* __restrict__ grad_loss, float* __restrict__ grad_preds,
                                                           int n_iter, int B, int hw, double gamma) {
    const long long npix = (long long)B * hw;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (q >= npix) return;
    const int b = (int)(q / hw), yx = (int)(q - (long long)b * hw);
    const size_t o = ((size_t)(i * B + b) * 2) * hw + yx;
    float gmu = 0.f, gsig = 0.f;
    if (mask[q]) {
        const float scale = (float)((double)(*grad_loss) * pow(gamma, (double)(n_iter - 1 - i)) / sums[0]);
        const float mu = preds[o], sigma = preds[o + hw];
        bool cl;
        const float var = nll_var(sigma, cl);
        const float d = mu - gt[q];
        gmu = scale * (d / var);
        gsig = cl ? 0.f : scale * ((0.5f / var - d * d / (2.f * var * var)) * (2.f * sigma));
    }
    grad_preds[o] = gmu;
    grad_preds[o + hw] = gsig;
}

hipError_t launch_nll_forward(const MagnetNllArgs& a, hipStream_t s) {
    const int hw = a.H * a.W;
    hipLaunchKernelGGL(nll_partial_kernel, dim3(NLL_BLOCKS), dim3(256), 0, s, a.preds, a.gt, a.mask, a.work, a.n_iter, a.B, hw);
    hipLaunchKernelGGL(nll_final_kernel, dim3(1), dim3(64), 0, s, a.work, a.sums, a.loss, a.n_iter, a.gamma);
    return hipGetLastError();
}

hipError_t launch_nll_backward(const MagnetNllArgs& a, hipStream_t s) {
    const int hw = a.H * a.W;
    const long long npix = (long long)a.B * hw;
    hipLaunchKernelGGL(nll_backward_kernel, dim3((unsigned)((npix + 255) / 256), a.n_iter), dim3(256), 0, s, a.preds, a.gt, a.mask,
                       a.sums, a.grad_loss, a.grad_preds, a.n_iter, a.B, hw, a.gamma);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Convex-upsampling backward (models/MAGNET.py:15-27).  Forward: up[n,b,c, y*k+i, x*k+j] = sum_t p_t * depth[n,b,c, y+dy_t, x+dx_t]
// (zero outside), p = softmax_t(mask[b, t*k*k + i*k + j, y, x]), t = 3*(dy+1) + (dx+1) (nn.functional.unfold order).
// ---------------------------------------------------------------------------------------------------------------------
struct UpBwd {
    const float* gup; const float* depth; const float* mask; float* gdepth; float* gmask; float* part;
    long long sb, sc, sy, sx, gsb, gsc, gsy, gsx;
    int n, B, h, w, k;
};

__device__ __forceinline__ void up_softmax(const UpBwd& a, const float* mb, int sub, float p[9]) {
    const int kk = a.k * a.k;
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 9; ++t) { p[t] = mb[(long long)(t * kk + sub) * a.sc]; m = fmaxf(m, p[t]); }
    float z = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) { p[t] = expf(p[t] - m); z += p[t]; }
#pragma unroll
    for (int t = 0; t < 9; ++t) p[t] = p[t] / z;
}

// pass 1: one thread per low-resolution pixel: d mask (all sub-pixels, summed over iterations) and, per (iteration, channel,
// tap), sum over the k*k sub-pixels of p_t * d up -> part (n, B, 2, 9, h, w)
__global__ __launch_bounds__(256) void upbwd_pixel_kernel(const UpBwd a) {
    const int hw = a.h * a.w;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)a.B * hw) return;
    const int b = (int)(q / hw), yx = (int)(q - (long long)b * hw), y = yx / a.w, x = yx - y * a.w;
    const int k = a.k, kk = k * k, H = k * a.h, W = k * a.w;
    const float* mb = a.mask + b * a.sb + y * a.sy + x * a.sx;
    float* gb = a.gmask + b * a.gsb + y * a.gsy + x * a.gsx;
    // the 3x3 zero-padded patches of every (iteration, channel) are re-read per sub-pixel (L1-resident)
    for (int sub = 0; sub < kk; ++sub) {
        const int i = sub / k, j = sub - i * k;
        float p[9], G[9];
        up_softmax(a, mb, sub, p);
#pragma unroll
        for (int t = 0; t < 9; ++t) G[t] = 0.f;
        for (int n = 0; n < a.n; ++n)
            for (int c = 0; c < 2; ++c) {
                const size_t img = (size_t)(n * a.B + b) * 2 + c;
                const float g = a.gup[img * H * W + (size_t)(y * k + i) * W + x * k + j];
                const float* d = a.depth + img * hw;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
                    const float v = (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) ? d[yy * a.w + xx] : 0.f;
                    G[t] += g * v;
                }
            }
        float pg = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) pg += p[t] * G[t];
#pragma unroll
        for (int t = 0; t < 9; ++t) gb[(long long)(t * kk + sub) * a.gsc] = p[t] * (G[t] - pg);
    }
    for (int n = 0; n < a.n; ++n)
        for (int c = 0; c < 2; ++c) {
            const size_t img = (size_t)(n * a.B + b) * 2 + c;
            float acc[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[t] = 0.f;
            for (int sub = 0; sub < kk; ++sub) {
                const int i = sub / k, j = sub - i * k;
                float p[9];
                up_softmax(a, mb, sub, p);
                const float g = a.gup[img * H * W + (size_t)(y * k + i) * W + x * k + j];
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[t] += p[t] * g;
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) a.part[(img * 9 + t) * hw + yx] = acc[t];
        }
}

// pass 2: d depth[n,b,c,Y,X] = sum_t part[n,b,c,t, Y-dy_t, X-dx_t] (fixed tap order; sources outside the grid contribute nothing)
__global__ __launch_bounds__(256) void upbwd_gather_kernel(const UpBwd a) {
    const int hw = a.h * a.w;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)a.n * a.B * 2 * hw) return;
    const size_t img = (size_t)(q / hw);
    const int yx = (int)(q - (long long)img * hw), Y = yx / a.w, X = yx - Y * a.w;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int y = Y - (t / 3 - 1), x = X - (t % 3 - 1);
        if (y >= 0 && y < a.h && x >= 0 && x < a.w) s += a.part[(img * 9 + t) * hw + y * a.w + x];
    }
    a.gdepth[q] = s;
}

hipError_t launch_upsample_backward(const MagnetUpsampleBwdArgs& u, hipStream_t s) {
    UpBwd a{u.grad_up, u.depth, u.mask, u.grad_depth, u.grad_mask, u.work, u.mask_sb, u.mask_sc, u.mask_sy, u.mask_sx,
            u.gm_sb, u.gm_sc, u.gm_sy, u.gm_sx, u.n_pred, u.B, u.h, u.w, u.k};
    const long long npix = (long long)u.B * u.h * u.w;
    hipLaunchKernelGGL(upbwd_pixel_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, a);
    const long long nout = (long long)u.n_pred * 2 * npix;
    hipLaunchKernelGGL(upbwd_gather_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Head backward: the 1x1 tail of a stack, transposed (dgrad).  Workgroup = 128 rows (4 waves x 32 rows, rows are wave-private),
// MFMA operands swapped as in conv_mfma.hip's tail: A = W^T fragment (rows = input channels of the forward layer, K = its output
// channels, straight from global / L2), B = gradient fragment (K = channels, columns = tile rows); the accumulator is C^T, a
// lane holds 4 consecutive channels of one row.  Layer 1 reads dout from global (or computes it: G-Net's Gaussian update
// backward), layers 2 and 3 read the previous gradient tile from LDS (conv_mfma's act_swz image, 256 B per row and plane).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int dg_swz(int row, int slot) { return row * 256 + ((slot ^ (row & 15)) << 4); }

__device__ __forceinline__ bool dg_border(long long p, int h, int w) {
    const int wp = w + 2, hp = h + 2;
    const long long img = p / ((long long)hp * wp);
    const int r = (int)(p - img * hp * wp), y = r / wp, x = r - y * wp;
    return y == 0 || y == hp - 1 || x == 0 || x == wp - 1;
}

template <int KS>   // KS = K steps of 32 channels of this layer
__device__ __forceinline__ void dg_mma(f32x4_t (&acc)[8][2], const uint16_t* __restrict__ wt_hi, const uint16_t* __restrict__ wt_lo,
                                       const bf16x8_t (&bh)[KS][2], const bf16x8_t (&bl)[KS][2], int lane) {
    const int frow = lane & 15, q = lane >> 4;
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[n][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const size_t e = (size_t)(n * 16 + frow) * (KS * 32) + kk * 32 + q * 8;
            const bf16x8_t wh = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(wt_hi + e));
            const bf16x8_t wl = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(wt_lo + e));
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, bl[kk][m], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, bh[kk][m], acc[n][m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, bh[kk][m], acc[n][m], 0, 0, 0);
        }
}

// acc (C^T) -> ReLU-mask by the forward activation, zero border rows, write the split planes to global (and the accumulated fp32
// sum for the last layer), and the tile into LDS for the next product
__device__ __forceinline__ void dg_epilogue(const MagnetHeadDgradArgs& a, f32x4_t (&acc)[8][2], const uint16_t* __restrict__ h_hi,
                                            uint16_t* __restrict__ o_hi, uint16_t* __restrict__ o_lo, bool last,
                                            unsigned char* act_hi, unsigned char* act_lo, long long row0, int lane, int wv) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int ch = n * 16 + (lane >> 4) * 4;
            const int trow = wv * 32 + m * 16 + (lane & 15);
            const long long p = row0 + trow;
            float v[4] = {acc[n][m][0], acc[n][m][1], acc[n][m][2], acc[n][m][3]};
            const bool live = p < a.rows && !dg_border(p, a.h, a.w);
            if (live) {
                const uint2 hb = *reinterpret_cast<const uint2*>(h_hi + (size_t)p * 128 + ch);
                const uint32_t hv[4] = {hb.x & 0xffffu, hb.x >> 16, hb.y & 0xffffu, hb.y >> 16};
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (__uint_as_float(hv[r] << 16) > 0.f) ? v[r] : 0.f;   // [h > 0]
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = 0.f;
            }
            uint32_t h01, l01, h23, l23;
            split_bf16x2(v[0], v[1], h01, l01); split_bf16x2(v[2], v[3], h23, l23);
            if (p < a.rows) {
                *reinterpret_cast<uint2*>(o_hi + (size_t)p * 128 + ch) = make_uint2(h01, h23);
                *reinterpret_cast<uint2*>(o_lo + (size_t)p * 128 + ch) = make_uint2(l01, l23);
                if (last && a.acc) {
                    float4* ap = reinterpret_cast<float4*>(a.acc + (size_t)p * 128 + ch);
                    float4 s = make_float4(v[0], v[1], v[2], v[3]);
                    if (a.acc_mode == 2) { const float4 o = *ap; s = make_float4(o.x + v[0], o.y + v[1], o.z + v[2], o.w + v[3]); }
                    *ap = s;
                    if (a.acc_hi) {
                        uint32_t ah01, al01, ah23, al23;
                        split_bf16x2(s.x, s.y, ah01, al01); split_bf16x2(s.z, s.w, ah23, al23);
                        *reinterpret_cast<uint2*>((uint16_t*)a.acc_hi + (size_t)p * 128 + ch) = make_uint2(ah01, ah23);
                        *reinterpret_cast<uint2*>((uint16_t*)a.acc_lo + (size_t)p * 128 + ch) = make_uint2(al01, al23);
                    }
                }
            }
            if (!last) {
                const int off = dg_swz(trow, ch >> 3) + (ch & 7) * 2;
                *reinterpret_cast<uint2*>(act_hi + off) = make_uint2(h01, h23);
                *reinterpret_cast<uint2*>(act_lo + off) = make_uint2(l01, l23);
            }
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void dg_lds_frags(bf16x8_t (&bh)[4][2], bf16x8_t (&bl)[4][2], const unsigned char* act_hi,
                                             const unsigned char* act_lo, int lane, int wv) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int row = wv * 32 + m * 16 + (lane & 15);
            bh[kk][m] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(act_hi + dg_swz(row, kk * 4 + (lane >> 4))));
            bl[kk][m] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(act_lo + dg_swz(row, kk * 4 + (lane >> 4))));
        }
}

template <int KS0>
__global__ __launch_bounds__(256) void dgrad_kernel(const MagnetHeadDgradArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char act[2 * 128 * 256];
    unsigned char* act_hi = act;
    unsigned char* act_lo = act + 128 * 256;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4;
    const long long row0 = (long long)blockIdx.x * 128;
    const int K0 = KS0 * 32;
    // ---- layer 4^T: B fragments of dout (split on the fly), also written out as split planes for dW4 ----
    bf16x8_t bh0[KS0][2], bl0[KS0][2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const long long p = row0 + wv * 32 + m * 16 + (lane & 15);
        const bool inb = p < a.rows;
        float g0 = 0.f, g1 = 0.f;
        if (!a.dout && inb && !dg_border(p, a.h, a.w)) {
            // G-Net: Gaussian update backward (models/MAGNET.py:60-69): mu = mu0 + o0*s0, sigma = (elu(o1) + 1 + 1e-10)*s0
            const int wp = a.w + 2, hp = a.h + 2;
            const long long img = p / ((long long)hp * wp);
            const int r = (int)(p - img * hp * wp), y = r / wp - 1, x = r % wp - 1;
            const size_t e = ((size_t)img * 2) * a.h * a.w + (size_t)y * a.w + x, hw = (size_t)a.h * a.w;
            const float s0 = a.gmm_in[e + hw];
            const float o1 = a.gnet_out[(size_t)p * a.gnet_ld + 1];
            g0 = a.grad_gmm[e] * s0;
            g1 = a.grad_gmm[e + hw] * (o1 > 0.f ? 1.f : expf(o1)) * s0;
        }
#pragma unroll
        for (int kk = 0; kk < KS0; ++kk) {
            const int c = kk * 32 + q * 8;
            float v[8];
            if (a.dout) {
                if (inb) {
                    const float4 u0 = *reinterpret_cast<const float4*>(a.dout + (size_t)p * K0 + c);
                    const float4 u1 = *reinterpret_cast<const float4*>(a.dout + (size_t)p * K0 + c + 4);
                    v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[r] = 0.f;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = 0.f;
                if (c == 0) { v[0] = g0; v[1] = g1; }
            }
            uint4 hq, lq;
            split_bf16x2(v[0], v[1], hq.x, lq.x); split_bf16x2(v[2], v[3], hq.y, lq.y);
            split_bf16x2(v[4], v[5], hq.z, lq.z); split_bf16x2(v[6], v[7], hq.w, lq.w);
            bh0[kk][m] = __builtin_bit_cast(bf16x8_t, hq);
            bl0[kk][m] = __builtin_bit_cast(bf16x8_t, lq);
            if (inb) {
                *reinterpret_cast<uint4*>((uint16_t*)a.dout_hi + (size_t)p * K0 + c) = hq;
                *reinterpret_cast<uint4*>((uint16_t*)a.dout_lo + (size_t)p * K0 + c) = lq;
            }
        }
    }
    const uint16_t* wt_hi = (const uint16_t*)a.wt_hi;
    const uint16_t* wt_lo = (const uint16_t*)a.wt_lo;
    f32x4_t acc[8][2];
    dg_mma<KS0>(acc, wt_hi, wt_lo, bh0, bl0, lane);
    dg_epilogue(a, acc, (const uint16_t*)a.h3_hi, (uint16_t*)a.dh3_hi, (uint16_t*)a.dh3_lo, false, act_hi, act_lo, row0, lane, wv);
    // ---- layer 3^T ----
    bf16x8_t bh[4][2], bl[4][2];
    dg_lds_frags(bh, bl, act_hi, act_lo, lane, wv);
    dg_mma<4>(acc, wt_hi + 128 * K0, wt_lo + 128 * K0, bh, bl, lane);
    dg_epilogue(a, acc, (const uint16_t*)a.h2_hi, (uint16_t*)a.dh2_hi, (uint16_t*)a.dh2_lo, false, act_hi, act_lo, row0, lane, wv);
    // ---- layer 2^T ----
    dg_lds_frags(bh, bl, act_hi, act_lo, lane, wv);
    dg_mma<4>(acc, wt_hi + 128 * K0 + 128 * 128, wt_lo + 128 * K0 + 128 * 128, bh, bl, lane);
    dg_epilogue(a, acc, (const uint16_t*)a.h1_hi, (uint16_t*)a.dh1_hi, (uint16_t*)a.dh1_lo, true, act_hi, act_lo, row0, lane, wv);
}

hipError_t launch_head_dgrad(const MagnetHeadDgradArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows + 127) / 128));
    switch (a.k0) {
        case 32:  hipLaunchKernelGGL(dgrad_kernel<1>, grid, dim3(256), 0, s, a); break;
        case 128: hipLaunchKernelGGL(dgrad_kernel<4>, grid, dim3(256), 0, s, a); break;
        case 160: hipLaunchKernelGGL(dgrad_kernel<5>, grid, dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient.  Workgroup tile: 64 output channels (o) x 64 input channels (c) of one tap over one chunk of WG_CHUNK rows;
// 2 x 2 waves of 32 x 32.  Per K step of 32 rows the dY (rows x 64 o) and X (rows x 64 c) tiles are staged row-major in LDS
// (128-byte rows, 16-byte chunks XOR-swizzled by row) and both MFMA operands are read with ds_read_b64_tr_b16: lane 4qq+pp of a
// 16-lane group g supplies row 8g + 4h + qq, columns 4pp..4pp+3 of its 16-column block and receives column (lane & 15) of the
// 4 rows — the operand map A[i = lane & 15][k = 8g + j] of v_mfma_f32_16x16x32_bf16 (h = 0: j = 0..3, h = 1: j = 4..7).
// ---------------------------------------------------------------------------------------------------------------------
struct WgradP {
    const uint16_t *dy_hi, *dy_lo, *x_hi, *x_lo;
    long long dy_ld, x_ld;
    int cout, cin, taps, wp, ntc, nto;
    long long p0, p1;           // summed rows [p0, p1)
    float* part;                // [chunk][tap][cout][cin]
    long long toff[9];          // row offset of each tap
};

__device__ __forceinline__ int wg_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

__device__ __forceinline__ s16x4_t wg_tr(const unsigned char* base, int row, int col) {
    // 4 columns col..col+3 of `row` (col % 4 == 0): 8 bytes inside one 16-byte chunk
    const unsigned char* ptr = base + wg_off(row, col >> 3) + (col & 7) * 2;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(ptr));
}

__device__ __forceinline__ bf16x8_t wg_frag(const unsigned char* img, int col0, int lane) {
    const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const s16x4_t lo4 = wg_tr(img, 8 * g + qq, col0 + 4 * pp);
    const s16x4_t hi4 = wg_tr(img, 8 * g + 4 + qq, col0 + 4 * pp);
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    const s16x8_t v = s16x8_t{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}

__global__ __launch_bounds__(256) void wgrad_kernel(const WgradP a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[4][32 * 128];   // dY hi, dY lo, X hi, X lo
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int t = blockIdx.x;
    const int tc = t % a.ntc; t /= a.ntc;
    const int to = t % a.nto; t /= a.nto;
    const int tap = t;
    const int chunk = blockIdx.y;
    const long long off = a.toff[tap];
    const int o0 = to * 64, c0 = tc * 64;
    const long long pb = a.p0 + (long long)chunk * WG_CHUNK;
    const long long pe = pb + WG_CHUNK < a.p1 ? pb + WG_CHUNK : a.p1;
    // staging: thread -> (row sr = tid / 8, 16-byte chunk sq = tid % 8) of both 32 x 64 tiles
    const int sr = tid >> 3, sq = tid & 7;
    const int wo = wv & 1, wc = wv >> 1;
    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (long long k0 = pb; k0 < pe; k0 += 32) {
        const long long p = k0 + sr;
        uint4 yh = make_uint4(0, 0, 0, 0), yl = yh, xh = yh, xl = yh;
        if (p < pe) {
            const int oc = o0 + sq * 8, cc = c0 + sq * 8;
            if (oc < a.cout) {
                yh = *reinterpret_cast<const uint4*>(a.dy_hi + p * a.dy_ld + oc);
                yl = *reinterpret_cast<const uint4*>(a.dy_lo + p * a.dy_ld + oc);
            }
            if (cc < a.cin) {
                xh = *reinterpret_cast<const uint4*>(a.x_hi + (p + off) * a.x_ld + cc);
                xl = *reinterpret_cast<const uint4*>(a.x_lo + (p + off) * a.x_ld + cc);
            }
        }
        __syncthreads();                                                   // previous step's reads are done
        *reinterpret_cast<uint4*>(lds[0] + wg_off(sr, sq)) = yh;
        *reinterpret_cast<uint4*>(lds[1] + wg_off(sr, sq)) = yl;
        *reinterpret_cast<uint4*>(lds[2] + wg_off(sr, sq)) = xh;
        *reinterpret_cast<uint4*>(lds[3] + wg_off(sr, sq)) = xl;
        __syncthreads();
        bf16x8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[i] = wg_frag(lds[0], wo * 32 + i * 16, lane);
            al[i] = wg_frag(lds[1], wo * 32 + i * 16, lane);
            bh[i] = wg_frag(lds[2], wc * 32 + i * 16, lane);
            bl[i] = wg_frag(lds[3], wc * 32 + i * 16, lane);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            }
    }
    // D[o][c]: lane holds c = (lane & 15), o = (lane >> 4) * 4 + r of each 16 x 16 block
    float* dst = a.part + ((size_t)chunk * a.taps + tap) * a.cout * a.cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + wc * 32 + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + wo * 32 + i * 16 + (lane >> 4) * 4 + r;
                if (o < a.cout && c < a.cin) dst[(size_t)o * a.cin + c] = acc[i][j][r];
            }
        }
}

// bias partial sums: column sums of dY (hi + lo) over each chunk.  Workgroup = one chunk x 16 columns; 16 row lanes per column sum
// rows r, r + 16, ... in order, then lane 0 adds the 16 lane sums in order
__global__ __launch_bounds__(256) void wgrad_bias_kernel(const WgradP a, float* __restrict__ bpart) {
    __shared__ float red[16][17];
    const long long pb = a.p0 + (long long)blockIdx.x * WG_CHUNK;
    const long long pe = pb + WG_CHUNK < a.p1 ? pb + WG_CHUNK : a.p1;
    const int col = threadIdx.x & 15, lr = threadIdx.x >> 4;
    const int o = blockIdx.y * 16 + col;
    float s = 0.f;
    if (o < a.cout)
        for (long long p = pb + lr; p < pe; p += 16)
            s += bf16_to_f32(a.dy_hi[p * a.dy_ld + o]) + bf16_to_f32(a.dy_lo[p * a.dy_ld + o]);
    red[lr][col] = s;
    __syncthreads();
    if (lr == 0 && o < a.cout) {
        float t = 0.f;
        for (int r = 0; r < 16; ++r) t += red[r][col];
        bpart[(size_t)blockIdx.x * a.cout + o] = t;
    }
}

// fixed-order sum over the chunks, mapped into nn.Conv2d's (cout_total = any, cin_total, taps) layout
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WgradP a, int nchunks, const MagnetWgradArgs g, const float* __restrict__ bpart) {
    const long long n = (long long)a.taps * g.cout_valid * g.cin_valid;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int c = (int)(i % g.cin_valid);
        const long long r = i / g.cin_valid;
        const int o = (int)(r % g.cout_valid), tap = (int)(r / g.cout_valid);
        float s = 0.f;
        for (int k = 0; k < nchunks; ++k) s += a.part[(((size_t)k * a.taps + tap) * a.cout + o) * a.cin + c];
        float* d = g.grad_w + ((size_t)o * g.cin_total + g.cin_dst + c) * a.taps + tap;
        *d = g.accumulate ? *d + s : s;
    }
    if (g.grad_b && i < g.cout_valid) {
        float s = 0.f;
        for (int k = 0; k < nchunks; ++k) s += bpart[(size_t)k * a.cout + i];
        g.grad_b[i] = g.accumulate ? g.grad_b[i] + s : s;
    }
}

int wgrad_chunks(const MagnetWgradArgs& g) {
    const long long p0 = g.wp + 1, p1 = g.rows - g.wp - 1;
    return p1 > p0 ? (int)((p1 - p0 + WG_CHUNK - 1) / WG_CHUNK) : 0;
}

long long wgrad_workspace_bytes(const MagnetWgradArgs& g) {
    const long long nc = wgrad_chunks(g);
    return 4 * nc * ((long long)g.taps * g.cout * g.cin + g.cout);
}

hipError_t launch_wgrad(const MagnetWgradArgs& g, hipStream_t s) {
    const int nch = wgrad_chunks(g);
    WgradP a{(const uint16_t*)g.dy_hi, (const uint16_t*)g.dy_lo, (const uint16_t*)g.x_hi, (const uint16_t*)g.x_lo, g.dy_ld, g.x_ld,
             g.cout, g.cin, g.taps, g.wp, (g.cin + 63) / 64, (g.cout + 63) / 64, (long long)g.wp + 1, g.rows - g.wp - 1, g.work, {}};
    for (int t = 0; t < g.taps; ++t) a.toff[t] = g.taps == 9 ? (long long)(t / 3 - 1) * g.wp + (t % 3 - 1) : 0;
    float* bpart = g.work + (size_t)nch * g.taps * g.cout * g.cin;
    if (nch > 0) {
        hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)(a.ntc * a.nto * g.taps), nch), dim3(256), 0, s, a);
        if (g.grad_b) hipLaunchKernelGGL(wgrad_bias_kernel, dim3(nch, (g.cout + 15) / 16), dim3(256), 0, s, a, bpart);
    }
    const long long n = (long long)g.taps * g.cout_valid * g.cin_valid;
    const long long nt = n > g.cout_valid ? n : g.cout_valid;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, a, nch, g, bpart);
    return hipGetLastError();
}

// magnet_wgrad_ex: the same kernels with the tap offsets of a dilated 3x3 (taps 9, dil), of the space-to-depth 2x2 window
// (taps 4: offsets -wp-1, -wp, -1, 0) or of a 1x1, summed over the rows [max(0, -min off), rows - max(0, max off)): every read stays
// inside the grid, and dy is zero on the border rows the range leaves out
static void wgrad_ex_range(const MagnetWgradExArgs& e, long long* toff, long long& p0, long long& p1) {
    const MagnetWgradArgs& g = e.base;
    const int d = e.dil > 1 ? e.dil : 1;
    long long mn = 0, mx = 0;
    for (int t = 0; t < g.taps; ++t) {
        toff[t] = g.taps == 9 ? ((long long)(t / 3 - 1) * g.wp + (t % 3 - 1)) * d
                : (g.taps == 4 ? (t == 0 ? -(long long)g.wp - 1 : (t == 1 ? -(long long)g.wp : (t == 2 ? -1 : 0))) : 0);
        mn = toff[t] < mn ? toff[t] : mn;
        mx = toff[t] > mx ? toff[t] : mx;
    }
    p0 = -mn;
    p1 = g.rows - mx;
}

int wgrad_ex_chunks(const MagnetWgradExArgs& e) {
    long long toff[9], p0, p1;
    wgrad_ex_range(e, toff, p0, p1);
    return p1 > p0 ? (int)((p1 - p0 + WG_CHUNK - 1) / WG_CHUNK) : 0;
}

long long wgrad_ex_workspace_bytes(const MagnetWgradExArgs& e) {
    const long long nc = wgrad_ex_chunks(e);
    return 4 * nc * ((long long)e.base.taps * e.base.cout * e.base.cin + e.base.cout);
}

hipError_t launch_wgrad_ex(const MagnetWgradExArgs& e, hipStream_t s) {
    const MagnetWgradArgs& g = e.base;
    const int nch = wgrad_ex_chunks(e);
    WgradP a{(const uint16_t*)g.dy_hi, (const uint16_t*)g.dy_lo, (const uint16_t*)g.x_hi, (const uint16_t*)g.x_lo, g.dy_ld, g.x_ld,
             g.cout, g.cin, g.taps, g.wp, (g.cin + 63) / 64, (g.cout + 63) / 64, 0, 0, g.work, {}};
    wgrad_ex_range(e, a.toff, a.p0, a.p1);
    float* bpart = g.work + (size_t)nch * g.taps * g.cout * g.cin;
    if (nch > 0) {
        hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)(a.ntc * a.nto * g.taps), nch), dim3(256), 0, s, a);
        if (g.grad_b) hipLaunchKernelGGL(wgrad_bias_kernel, dim3(nch, (g.cout + 15) / 16), dim3(256), 0, s, a, bpart);
    }
    const long long n = (long long)g.taps * g.cout_valid * g.cin_valid;
    const long long nt = n > g.cout_valid ? n : g.cout_valid;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, a, nch, g, bpart);
    return hipGetLastError();
}

}  // namespace magnet
