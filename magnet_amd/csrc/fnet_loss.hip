// fnet_loss.hip — the tail of the F-Net training step (reference train_FNet.py:95-104) and of its validate() (train_FNet.py:166-167)
// on the raw matching volume x (B, D, h, w) that the mode-1 matcher writes: softmax over the D depth bins, expected depth under the
// bin centres d, masked L1 loss against the ground truth, and the gradient back to x.
//
//   fnl_pred_kernel      per pixel, one pass over the D logits in ascending order (each read once): the online form in chunks of
//                        CH bins: mn = max(m, chunk max); Z and S are rescaled by expf(m - mn) (exactly 1 when the maximum did not
//                        move), then Z += e_j, S = fma(e_j, d_j, S) with e_j = expf(x_j - mn).  pred = S / Z; m and 1 / Z are kept for
//                        the backward.
//   fnl_partial / _final the loss: count and sum of |pred - gt| over the valid pixels in fp64, the fixed-grid two-stage scheme of
//                        nll_partial_kernel / nll_final_kernel (train_bwd.hip): NLL_BLOCKS workgroups with a grid-stride loop, then one
//                        fixed-order sum.  No atomics: bit-identical from run to run.
//   fnl_backward_kernel  grad_x_j = g p_j (d_j - pred), p_j = expf(x_j - m) / Z recomputed, g = grad_loss / count * sign(pred - gt)
//                        on valid pixels and 0 elsewhere; grad_loss and count are read on the device.  One read of x, one write of
//                        grad_x; a wave with no pixel of non-zero g stores zeros without reading x.
//
// Mapping: thread = pixel, consecutive lanes = consecutive pixels, so every bin plane is read (and written) as full 256-byte wave
// rows; one wave per workgroup (no LDS, no barrier), which spreads the 4 800 waves of the training shape (16 x 120 x 160) evenly over the
// 256 CUs.  With a handful of waves per SIMD the memory pipes are filled from inside a lane: the CH loads of a chunk are independent
// and issued together.  d is indexed uniformly and read through the scalar cache.  Both kernels stream the volume once per direction (forward
// 4 BDhw + 12 Bhw, backward 8 BDhw + 12 Bhw bytes) at ~25 vector instructions per element, so expf is the accurate one, as in
// dnet_upsample_gauss_kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"

namespace magnet {

namespace {

constexpr int FNL_BLOCKS = MAGNET_NLL_BLOCKS;
constexpr int CH = 16;                                   // bins per chunk = independent loads in flight per lane

__device__ __forceinline__ bool fnl_valid(float gt, float min_depth, float max_depth) {
    return gt > min_depth && !(gt > max_depth);          // gt[gt > max_depth] = 0; mask = gt > min_depth  (min_depth >= 0); NaN: invalid
}

__global__ __launch_bounds__(64) void fnl_pred_kernel(const float* __restrict__ x, const float* __restrict__ d, float* __restrict__ pred,
                                                      float* __restrict__ m_out, float* __restrict__ rz_out, int D, long long hw,
                                                      long long npix) {
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
    if (q >= npix) return;
    const long long b = q / hw;
    const float* xp = x + (size_t)b * D * hw + (size_t)(q - b * hw);
    float m = -INFINITY, Z = 0.f, S = 0.f;
    int j = 0;
    for (; j + CH <= D; j += CH) {
        float v[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) v[k] = xp[(size_t)(j + k) * hw];
        float mn = m;
#pragma unroll
        for (int k = 0; k < CH; ++k) mn = fmaxf(mn, v[k]);
        const float sc = expf(m - mn);                   // 1 exactly when the maximum stays, 0 on the first chunk
        Z *= sc; S *= sc; m = mn;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const float e = expf(v[k] - m);
            Z += e;
            S = fmaf(e, d[j + k], S);
        }
    }
#pragma clang loop vectorize(disable)
    for (; j < D; ++j) {                                 // the last D % CH bins: chunks of one
        const float v = xp[(size_t)j * hw];
        const float mn = fmaxf(m, v);
        const float sc = expf(m - mn);
        Z *= sc; S *= sc; m = mn;
        const float e = expf(v - m);
        Z += e;
        S = fmaf(e, d[j], S);
    }
    pred[q] = S / Z;
    if (m_out) {
        m_out[q] = m;
        rz_out[q] = 1.0f / Z;
    }
}

__global__ __launch_bounds__(256) void fnl_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          double* __restrict__ work, long long npix, float min_depth, float max_depth) {
    __shared__ double red[2][256];
    double cnt = 0.0, sum = 0.0;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long long)FNL_BLOCKS * 256) {
        const float g = gt[q];
        if (!fnl_valid(g, min_depth, max_depth)) continue;
        cnt += 1.0;
        sum += (double)fabsf(pred[q] - g);
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

__global__ __launch_bounds__(64) void fnl_final_kernel(const double* __restrict__ work, double* __restrict__ sums, float* __restrict__ loss) {
    __shared__ double tot[2];
    const int t = threadIdx.x;
    if (t < 2) {
        double v = 0.0;
        for (int b = 0; b < FNL_BLOCKS; ++b) v += work[(size_t)b * 2 + t];     // fixed order
        tot[t] = v;
        sums[t] = v;
    }
    __syncthreads();
    if (t == 0) *loss = (float)(tot[1] / tot[0]);        // no valid pixel: 0 / 0 = NaN, as torch.mean of an empty selection
}

__global__ __launch_bounds__(64) void fnl_backward_kernel(const float* __restrict__ x, const float* __restrict__ d,
                                                          const float* __restrict__ gt, const float* __restrict__ pred,
                                                          const float* __restrict__ m_in, const float* __restrict__ rz_in,
                                                          const double* __restrict__ sums, const float* __restrict__ grad_loss,
                                                          float* __restrict__ grad_x, int D, long long hw, long long npix,
                                                          float min_depth, float max_depth) {
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
    if (q >= npix) return;
    const long long b = q / hw;
    const size_t o = (size_t)b * D * hw + (size_t)(q - b * hw);
    const float c = (float)((double)(*grad_loss) / sums[0]);
    const float gtv = gt[q], pr = pred[q];
    float g = 0.f;
    if (fnl_valid(gtv, min_depth, max_depth)) g = pr > gtv ? c : (pr < gtv ? -c : 0.f);      // sign(0) = 0 (torch's abs backward)
    float* gp = grad_x + o;
    if (__ballot(g != 0.f) == 0) {                       // wave-uniform: nothing but zeros here, x is not read
#pragma clang loop vectorize(disable)
        for (int j = 0; j < D; ++j) gp[(size_t)j * hw] = 0.f;
        return;
    }
    const float* xp = x + o;
    const float m = m_in[q];
    const float t = g * rz_in[q];
    int j = 0;
    for (; j + CH <= D; j += CH) {
        float v[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) v[k] = xp[(size_t)(j + k) * hw];
#pragma unroll
        for (int k = 0; k < CH; ++k) gp[(size_t)(j + k) * hw] = (t * expf(v[k] - m)) * (d[j + k] - pr);
    }
#pragma clang loop vectorize(disable)
    for (; j < D; ++j) gp[(size_t)j * hw] = (t * expf(xp[(size_t)j * hw] - m)) * (d[j] - pr);
}

}  // namespace

hipError_t launch_fnet_loss_forward(const MagnetFnetLossArgs& a, hipStream_t s) {
    const long long hw = (long long)a.h * a.w, npix = (long long)a.B * hw;
    hipLaunchKernelGGL(fnl_pred_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(64), 0, s, a.x, a.d, a.pred, a.gt ? a.m : nullptr,
                       a.gt ? a.rz : nullptr, a.D, hw, npix);
    if (a.gt) {
        hipLaunchKernelGGL(fnl_partial_kernel, dim3(FNL_BLOCKS), dim3(256), 0, s, a.pred, a.gt, a.work, npix, a.min_depth, a.max_depth);
        hipLaunchKernelGGL(fnl_final_kernel, dim3(1), dim3(64), 0, s, a.work, a.sums, a.loss);
    }
    return hipGetLastError();
}

hipError_t launch_fnet_loss_backward(const MagnetFnetLossArgs& a, hipStream_t s) {
    const long long hw = (long long)a.h * a.w, npix = (long long)a.B * hw;
    hipLaunchKernelGGL(fnl_backward_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(64), 0, s, a.x, a.d, a.gt, a.pred, a.m, a.rz, a.sums,
                       a.grad_loss, a.grad_x, a.D, hw, npix, a.min_depth, a.max_depth);
    return hipGetLastError();
}

}  // namespace magnet
