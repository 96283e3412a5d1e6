// Dev microbenchmark: the fp16 depthwise kernel of csrc/enc_kernels.hip (enc_dwconv_kernel<K, S, true>) with the channels per thread as a
// template parameter, 8 (one 16-byte load per pixel, the shipped form) against 16 (two), at the encoder's stage shapes for 1 and 5 images
// of 480 x 640.  Same tiling, arithmetic and order: the two outputs are compared bit for bit.  HIP events around each launch, 20 timed
// launches after 5 warm-up ones; prints the median and the minimum.  Result: profiles/encoder_precision/NOTES.md.
// Build: hipcc --offload-arch=gfx950 -O3 -o dw_channels dw_channels.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

constexpr int TH = 8, TW = 16;

__device__ __forceinline__ uint32_t f16_bits_sat(float x) {
    const float c = x != x ? x : __builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f);
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)c);
}
__device__ __forceinline__ uint4 f16x8_pack_sat(const float* v) {
    return make_uint4(f16_bits_sat(v[0]) | (f16_bits_sat(v[1]) << 16), f16_bits_sat(v[2]) | (f16_bits_sat(v[3]) << 16),
                      f16_bits_sat(v[4]) | (f16_bits_sat(v[5]) << 16), f16_bits_sat(v[6]) | (f16_bits_sat(v[7]) << 16));
}
__device__ __forceinline__ void f16x8_unpack(const uint4 u, float* v) {
    typedef __attribute__((ext_vector_type(8))) _Float16 h8_t;
    const h8_t h = __builtin_bit_cast(h8_t, u);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
}
__device__ __forceinline__ float silu_f32(float x) { return x / (1.0f + __builtin_amdgcn_exp2f(-x * 1.44269504088896341f)); }

struct P {
    const uint16_t* in; int in_ld, hi, wi, c_pad;
    const float* wgt; const float* bias;
    int pad_top, pad_left;
    uint16_t* out; int out_ld, ho, wo;
    float* part; int n_part;
};

template <int K, int S, int CPT>
__global__ __launch_bounds__(256) void dw_kernel(const P p) {
    extern __shared__ float red[];                            // [32 strips][cgb * CPT]
    const int cgb = blockDim.x >> 5;
    const int g = threadIdx.x % cgb, strip = threadIdx.x / cgb;
    const int tiles_x = (p.wo + TW - 1) / TW;
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int n = blockIdx.z;
    const int c = (blockIdx.y * cgb + g) * CPT;
    const int oy = ty * TH + (strip >> 2), ox0 = tx * TW + (strip & 3) * 4;
    const bool live = c < p.c_pad && oy < p.ho && ox0 < p.wo;
    float psum[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) psum[i] = 0.f;
    if (live) {
        float acc[4][CPT];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < CPT; ++i) acc[j][i] = 0.f;
        constexpr int SPAN = 3 * S + K;
        const int ix0 = ox0 * S - p.pad_left;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = oy * S + ky - p.pad_top;
            if (iy < 0 || iy >= p.hi) continue;
            float wk[K][CPT];
#pragma unroll
            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                for (int q = 0; q < CPT / 4; ++q) {
                    const float4 a = *reinterpret_cast<const float4*>(p.wgt + (size_t)(ky * K + kx) * p.c_pad + c + 4 * q);
                    wk[kx][4 * q] = a.x; wk[kx][4 * q + 1] = a.y; wk[kx][4 * q + 2] = a.z; wk[kx][4 * q + 3] = a.w;
                }
            const size_t rowbase = ((size_t)n * (p.hi + 2) + (iy + 1)) * (p.wi + 2) + 1;
#pragma unroll
            for (int t = 0; t < SPAN; ++t) {
                const int ix = ix0 + t;
                if (ix < 0 || ix >= p.wi) continue;
                float v[CPT];
#pragma unroll
                for (int q = 0; q < CPT / 8; ++q) f16x8_unpack(*reinterpret_cast<const uint4*>(p.in + (rowbase + ix) * p.in_ld + c + 8 * q), v + 8 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kx = t - j * S;
                    if (kx >= 0 && kx < K) {
#pragma unroll
                        for (int i = 0; i < CPT; ++i) acc[j][i] = __builtin_fmaf(wk[kx][i], v[i], acc[j][i]);
                    }
                }
            }
        }
        float bv[CPT];
#pragma unroll
        for (int q = 0; q < CPT / 4; ++q) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + c + 4 * q);
            bv[4 * q] = b.x; bv[4 * q + 1] = b.y; bv[4 * q + 2] = b.z; bv[4 * q + 3] = b.w;
        }
        const size_t orow = ((size_t)n * (p.ho + 2) + (oy + 1)) * (p.wo + 2) + 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ox0 + j >= p.wo) continue;
            float v[CPT];
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                v[i] = silu_f32(acc[j][i] + bv[i]);
                psum[i] += v[i];
            }
#pragma unroll
            for (int q = 0; q < CPT / 8; ++q) *reinterpret_cast<uint4*>(p.out + (orow + ox0 + j) * p.out_ld + c + 8 * q) = f16x8_pack_sat(v + 8 * q);
        }
    }
    const int cw = cgb * CPT;
#pragma unroll
    for (int i = 0; i < CPT; ++i) red[strip * cw + g * CPT + i] = psum[i];
    __syncthreads();
    for (int t = threadIdx.x; t < cw; t += blockDim.x) {
        const int ch = blockIdx.y * cw + t;
        if (ch < p.c_pad) {
            float s = red[t];
            for (int k = 1; k < 32; ++k) s += red[k * cw + t];
            p.part[((size_t)n * p.n_part + tile) * p.c_pad + ch] = s;
        }
    }
}

template <int K, int S, int CPT>
static void launch(const P& p, int N) {
    const int groups = p.c_pad / CPT;
    const int cgb = (groups % 8) == 0 ? 8 : ((groups % 4) == 0 ? 4 : 2);     // c_pad % 32 == 0: groups of 16 are a multiple of 2
    const dim3 grid((unsigned)p.n_part, (unsigned)(groups / cgb), (unsigned)N), block(32 * cgb);
    hipLaunchKernelGGL((dw_kernel<K, S, CPT>), grid, block, (size_t)32 * cgb * CPT * sizeof(float), 0, p);
}

template <int K, int S>
static void run_case(const char* name, int N, int h, int w, int c_pad) {
    const int ho = (h + S - 1) / S, wo = (w + S - 1) / S;
    const int pt = ((ho - 1) * S + K - h > 0 ? (ho - 1) * S + K - h : 0) / 2, pl = ((wo - 1) * S + K - w > 0 ? (wo - 1) * S + K - w : 0) / 2;
    const size_t n_in = (size_t)N * (h + 2) * (w + 2) * c_pad, n_out = (size_t)N * (ho + 2) * (wo + 2) * c_pad;
    const int n_part = ((ho + TH - 1) / TH) * ((wo + TW - 1) / TW);
    std::vector<uint16_t> hin(n_in);
    for (size_t i = 0; i < n_in; ++i) hin[i] = (uint16_t)(0x3000 + (rand() % 0x0c00)) | (uint16_t)((rand() & 1) << 15);     // |x| in [0.125, 1)
    std::vector<float> hw((size_t)K * K * c_pad), hb(c_pad);
    for (auto& v : hw) v = (rand() % 2001 - 1000) * 4e-4f;
    for (auto& v : hb) v = (rand() % 2001 - 1000) * 3e-4f;
    uint16_t *din, *dout[2]; float *dw, *db, *dpart[2];
    CK(hipMalloc(&din, n_in * 2)); CK(hipMalloc(&dw, hw.size() * 4)); CK(hipMalloc(&db, hb.size() * 4));
    for (int v = 0; v < 2; ++v) { CK(hipMalloc(&dout[v], n_out * 2)); CK(hipMemset(dout[v], 0, n_out * 2)); CK(hipMalloc(&dpart[v], (size_t)N * n_part * c_pad * 4)); }
    CK(hipMemcpy(din, hin.data(), n_in * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dw, hw.data(), hw.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float best[2] = {1e9f, 1e9f}, med[2];
    for (int v = 0; v < 2; ++v) {
        P p{din, c_pad, h, w, c_pad, dw, db, pt, pl, dout[v], c_pad, ho, wo, dpart[v], n_part};
        std::vector<float> ts;
        for (int it = 0; it < 25; ++it) {
            CK(hipEventRecord(e0));
            if (v == 0) launch<K, S, 8>(p, N); else launch<K, S, 16>(p, N);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (it >= 5) { ts.push_back(ms); if (ms < best[v]) best[v] = ms; }
        }
        std::sort(ts.begin(), ts.end()); med[v] = ts[ts.size() / 2];
    }
    std::vector<uint16_t> o0(n_out), o1(n_out);
    CK(hipMemcpy(o0.data(), dout[0], n_out * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(o1.data(), dout[1], n_out * 2, hipMemcpyDeviceToHost));
    size_t bad = 0; for (size_t i = 0; i < n_out; ++i) bad += o0[i] != o1[i];
    printf("%-28s N=%d %dx%d c_pad=%d k%d s%d: 8/thread median %.4f ms (min %.4f), 16/thread median %.4f ms (min %.4f), outputs differ at %zu\n", name, N, h, w,
           c_pad, K, S, med[0], best[0], med[1], best[1], bad);
    CK(hipFree(din)); CK(hipFree(dw)); CK(hipFree(db));
    for (int v = 0; v < 2; ++v) { CK(hipFree(dout[v])); CK(hipFree(dpart[v])); }
}

int main() {
    for (int N : {1, 5}) {
        run_case<3, 1>("stage 0 (48 ch, 240x320)", N, 240, 320, 64);
        run_case<3, 2>("stage 1.0 (144 ch, 240x320)", N, 240, 320, 160);
        run_case<3, 1>("stage 1.x (240 ch, 120x160)", N, 120, 160, 256);
        run_case<5, 2>("stage 2.0 (240 ch, 120x160)", N, 120, 160, 256);
        run_case<5, 1>("stage 2.x (384 ch, 60x80)", N, 60, 80, 384);
        run_case<3, 1>("stage 3.x (768 ch, 30x40)", N, 30, 40, 768);
        run_case<5, 1>("stage 4.x (1056 ch, 30x40)", N, 30, 40, 1152);
        run_case<5, 1>("stage 5.x (1824 ch, 15x20)", N, 15, 20, 1920);
        run_case<3, 1>("stage 6.x (3072 ch, 15x20)", N, 15, 20, 3072);
    }
    return 0;
}
