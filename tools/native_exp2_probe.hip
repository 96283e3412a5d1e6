// Dev probe: the error of the hardware exp2 instruction (v_exp_f32, __builtin_amdgcn_exp2f) that __expf is built on
// (__expf(x) = exp2(fl(x * log2e)) in clang's __clang_hip_math.h), over EVERY fp32 input in [-128, 0]: the range the softmax of
// upsample_kernel / upsample_cl_kernel feeds it (csrc/elementwise.hip).  One launch writes exp2 of all 0x43000001 inputs (-0.0 down
// to -128.0, 4.5 GB); the host compares each with fp64 exp2 and prints one JSON line:
//   max_ulp        worst |got - exact| / ulp(exact) over the inputs whose exact result is a normal fp32 (>= 2^-126)
//   max_sub_fmin   worst |got - exact| / 2^-126 over the inputs whose exact result is below 2^-126 (denormal results, kept or flushed)
// tests/elementwise_fwd_ref.py: E_NATIVE = max_ulp rounded up to the next whole ulp.  Not linked into the library.
//   hipcc --offload-arch=gfx950 -O2 tools/native_exp2_probe.hip -o tools/native_exp2_probe -lpthread && tools/native_exp2_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <thread>
#include <vector>

static const uint32_t kFirst = 0x80000000u;          // -0.0f
static const uint64_t kTotal = 0x43000000ull + 1;    // ... 0xC3000000 = -128.0f inclusive

__global__ __launch_bounds__(256) void exp2_all_kernel(float* __restrict__ out, uint64_t total) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256)
        out[i] = __builtin_amdgcn_exp2f(__uint_as_float(0x80000000u + (uint32_t)i));
}

struct Worst { double ulp = 0.0; uint32_t ulp_bits = 0; double sub = 0.0; uint32_t sub_bits = 0; uint64_t normal = 0, zeros_in_normal = 0; };

static void compare(const float* got, uint64_t i0, uint64_t n, Worst* w) {
    const double fmin = ldexp(1.0, -126);
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t bits = kFirst + (uint32_t)(i0 + k);
        float x;
        memcpy(&x, &bits, 4);
        const double exact = exp2((double)x);
        const double err = fabs((double)got[k] - exact);
        if (exact >= fmin) {
            const double e = err / ldexp(1.0, ilogb(exact) - 23);
            ++w->normal;
            if (got[k] == 0.f) ++w->zeros_in_normal;
            if (!(e <= w->ulp)) { w->ulp = e; w->ulp_bits = bits; }        // a NaN result counts as the worst
        } else {
            const double e = err / fmin;
            if (!(e <= w->sub)) { w->sub = e; w->sub_bits = bits; }
        }
    }
}

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    float* dev = nullptr;
    CK(hipMalloc(&dev, kTotal * sizeof(float)));
    hipLaunchKernelGGL(exp2_all_kernel, dim3(65536), dim3(256), 0, 0, dev, kTotal);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    const uint64_t chunk = 1ull << 26;
    const int nthreads = 16;
    std::vector<float> host(chunk);
    std::vector<Worst> worst(nthreads);
    for (uint64_t c0 = 0; c0 < kTotal; c0 += chunk) {
        const uint64_t n = kTotal - c0 < chunk ? kTotal - c0 : chunk;
        CK(hipMemcpy(host.data(), dev + c0, n * sizeof(float), hipMemcpyDeviceToHost));
        std::vector<std::thread> th;
        const uint64_t per = (n + nthreads - 1) / nthreads;
        for (int t = 0; t < nthreads; ++t) {
            const uint64_t a = (uint64_t)t * per, b = a + per < n ? a + per : n;
            if (a < b) th.emplace_back(compare, host.data() + a, c0 + a, b - a, &worst[t]);
        }
        for (auto& t : th) t.join();
        fprintf(stderr, "compared %llu / %llu\n", (unsigned long long)(c0 + n), (unsigned long long)kTotal);
    }
    CK(hipFree(dev));
    Worst w;
    for (const Worst& v : worst) {
        if (!(v.ulp <= w.ulp)) { w.ulp = v.ulp; w.ulp_bits = v.ulp_bits; }
        if (!(v.sub <= w.sub)) { w.sub = v.sub; w.sub_bits = v.sub_bits; }
        w.normal += v.normal; w.zeros_in_normal += v.zeros_in_normal;
    }
    float xu, xs;
    memcpy(&xu, &w.ulp_bits, 4); memcpy(&xs, &w.sub_bits, 4);
    printf("{\"inputs\": %llu, \"normal_results\": %llu, \"zero_where_normal\": %llu, \"max_ulp\": %.6f, \"max_ulp_at\": %.9g, "
           "\"max_sub_fmin\": %.6f, \"max_sub_at\": %.9g}\n", (unsigned long long)kTotal, (unsigned long long)w.normal,
           (unsigned long long)w.zeros_in_normal, w.ulp, (double)xu, w.sub, (double)xs);
    return 0;
}
