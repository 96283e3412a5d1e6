// frame_pool.hip — the frame pool's two data movers (magnet_amd/sequence.py), one launch each, both through a device table of slots:
// magnet_gather_views assembles a refinement step's inputs from the pool, magnet_scatter_frames (its inverse) writes the staged
// backbone outputs of new frames into the pool.  Pure data movement: every destination element is a copy of a source element, or
// (gather only) zero where the table names no frame.
//
// The work is cut into chunks of CHUNK 16-byte units.  A chunk lies inside one frame of one segment (gather: ref_cl, src_pad,
// ref_gmm, src_gmm, gin; scatter: feat, gmm, x_d3); a workgroup walks the chunks with a grid stride over a capped grid
// (walk_chunks, shared by both kernels), so every index computation that needs a division happens once per chunk on uniform values,
// and a thread's own work per unit is a shift or one 32-bit division by a uniform divisor.  No LDS, no atomics, ordinary vector
// loads and stores.
//
// Bounds: the slot of a chunk is read once and checked against [0, n_slots); outside that range nothing is read from the pool
// and zeros are stored (gather), or nothing is written at all (scatter).  Every pool offset is slot * frame + (offset inside one
// frame).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"

namespace magnet {

namespace {

constexpr int CHUNK = 2048;                // 16-byte units per chunk = 32 KiB: 8 units per thread of a 256-thread workgroup
constexpr int POOL_THREADS = 256;

enum { SEG_REF_CL = 0, SEG_SRC_PAD, SEG_REF_GMM, SEG_SRC_GMM, SEG_GIN, N_SEG };
enum { SC_FEAT = 0, SC_GMM, SC_XD3, N_SC };

template <int NSEG>
struct ChunkPlan {
    long long first[NSEG + 1];             // first chunk of each segment; first[NSEG] = all chunks
    int chunks_per_frame[NSEG];
    int units[NSEG];                       // units of one frame of the segment
};

// Fills the plan from the units of one frame and the number of frames of every segment; returns the number of chunks.
template <int NSEG>
long long plan_chunks(ChunkPlan<NSEG>& p, const long long* units, const long long* frames) {
    long long total = 0;
    for (int i = 0; i < NSEG; ++i) {
        p.first[i] = total;
        p.units[i] = (int)units[i];
        p.chunks_per_frame[i] = (int)((units[i] + CHUNK - 1) / CHUNK);
        total += frames[i] * p.chunks_per_frame[i];
    }
    p.first[NSEG] = total;
    return total;
}

// capped grid: 8 workgroups of 256 threads per compute unit of a 256-CU device keep the memory pipes full; more only adds
// launch and scheduling work
inline unsigned chunk_grid(long long total) {
    const long long cap = 256 * 8;
    return (unsigned)(total < cap ? total : cap);
}

// The grid-stride walk over the chunks of a plan: body(segment, frame inside the segment, first unit, end unit, units of a frame),
// all uniform over the workgroup.
template <int NSEG, typename Body>
__device__ __forceinline__ void walk_chunks(const ChunkPlan<NSEG>& p, Body body) {
    for (long long chunk = blockIdx.x; chunk < p.first[NSEG]; chunk += gridDim.x) {
        int seg = 0, cpf = 1, units = 0;
        long long c = 0;
#pragma unroll
        for (int i = 0; i < NSEG; ++i)                                // constant indices: the plan stays in scalar registers
            if (chunk >= p.first[i] && chunk < p.first[i + 1]) { seg = i; c = chunk - p.first[i]; cpf = p.chunks_per_frame[i]; units = p.units[i]; }
        const int e = (int)(c / cpf);                                 // frame inside the segment
        const int k = (int)(c - (long long)e * cpf);
        const int u0 = k * CHUNK;
        const int u1 = u0 + CHUNK < units ? u0 + CHUNK : units;
        body(seg, e, u0, u1, units);
    }
}

// One (mu, sigma) frame of n floats, for both kernels.  Frames are only 4-byte aligned in general (2 h w floats per frame, and the
// destination may be a view): when source and destination are misaligned by the same amount, unit 0 copies the floats up to the destination's first
// 16-byte boundary and unit k >= 1 the four floats behind it as one vector (the last one float by float where the frame ends inside
// it); otherwise every unit copies four floats one by one.
__device__ __forceinline__ void copy_gmm_unit(const float* __restrict__ src, float* __restrict__ dst, int n, int u, bool zero) {
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst);
    const bool same = zero || (((reinterpret_cast<uintptr_t>(src) ^ da) & 15u) == 0);
    int head = same ? (int)(((16u - (unsigned)(da & 15u)) & 15u) >> 2) : 0;
    head = head < n ? head : n;
    int lo, hi;
    if (u == 0) { lo = 0; hi = head; }
    else { lo = head + 4 * (u - 1); hi = lo + 4 < n ? lo + 4 : n; }
    if (lo >= hi) return;
    if (same && u > 0 && hi - lo == 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!zero) v = *reinterpret_cast<const float4*>(src + lo);
        *reinterpret_cast<float4*>(dst + lo) = v;
        return;
    }
    for (int i = lo; i < hi; ++i) {
        float v = 0.f;
        if (!zero) v = src[i];
        dst[i] = v;
    }
}

__global__ __launch_bounds__(POOL_THREADS) void gather_views_kernel(const MagnetGatherViewsArgs a, const ChunkPlan<N_SEG> p) {
    const int B = a.B;
    const int es = a.feat_dtype == MAGNET_FEAT_BF16 ? 2 : 4;
    const int R = (a.h + 2) * (a.w + 2);                              // rows of one padded frame
    const size_t feat_frame = (size_t)R * a.F * es;                   // bytes
    const int row_units = a.w * a.F * es / 16;                        // one interior row of ref_cl
    walk_chunks(p, [&](int seg, int e, int u0, int u1, int units) {
        const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
        // the table entry: [b] = reference of window b, [B + v B + b] = view v of window b
        int entry = e;
        if (seg == SEG_SRC_PAD || seg == SEG_SRC_GMM) entry = B + e;
        else if (seg == SEG_GIN) entry = e >= B ? e - B : e;          // frames [0, B) = hi plane, [B, 2B) = lo plane
        const int slot = a.slots[entry];
        const bool zero = slot < 0 || slot >= a.n_slots;
        const size_t s = zero ? 0 : (size_t)slot;
        // `zero` is uniform over the chunk: the zero fill and the copy are separate loops, so the copy's loads are plain global loads
        if (seg == SEG_REF_CL || seg == SEG_SRC_PAD) {
            const bool interior = seg == SEG_REF_CL;
            const char* src = static_cast<const char*>(a.pool_feat) + s * feat_frame;
            char* dst = static_cast<char*>(interior ? a.ref_cl : a.src_pad) + (size_t)e * units * 16;
            if (zero) {
                for (int u = u0 + threadIdx.x; u < u1; u += POOL_THREADS) *reinterpret_cast<uint4*>(dst + (size_t)u * 16) = zero4;
            } else if (interior) {                                    // row y of the interior starts one row and one texel into the frame
                for (int u = u0 + threadIdx.x; u < u1; u += POOL_THREADS) {
                    const int y = u / row_units, x = u - y * row_units;
                    const size_t off = ((size_t)(y + 1) * (a.w + 2) + 1) * a.F * es + (size_t)x * 16;
                    *reinterpret_cast<uint4*>(dst + (size_t)u * 16) = *reinterpret_cast<const uint4*>(src + off);
                }
            } else {
                for (int u = u0 + threadIdx.x; u < u1; u += POOL_THREADS)
                    *reinterpret_cast<uint4*>(dst + (size_t)u * 16) = *reinterpret_cast<const uint4*>(src + (size_t)u * 16);
            }
        } else if (seg == SEG_REF_GMM || seg == SEG_SRC_GMM) {
            const int n = 2 * a.h * a.w;
            const float* src = a.pool_gmm + s * n;
            float* dst = (seg == SEG_REF_GMM ? a.ref_gmm : a.src_gmm) + (size_t)e * n;
            for (int u = u0 + threadIdx.x; u < u1; u += POOL_THREADS) copy_gmm_unit(src, dst, n, u, zero);
        } else {
            const bool lo = e >= B;
            const int b = lo ? e - B : e;
            const char* src = static_cast<const char*>(lo ? a.pool_xd3_lo : a.pool_xd3_hi) + s * (size_t)R * 512;
            char* dst = static_cast<char*>(lo ? a.gin_lo : a.gin_hi) + ((size_t)b * R * a.gin_ld + a.gin_c_off) * 2;
            for (int u = u0 + threadIdx.x; u < u1; u += POOL_THREADS) {
                const int row = u >> 5, col = u & 31;                 // 256 bf16 channels = 32 units per row
                uint4 v = zero4;
                if (!zero) v = *reinterpret_cast<const uint4*>(src + (size_t)u * 16);
                *reinterpret_cast<uint4*>(dst + (size_t)row * a.gin_ld * 2 + col * 16) = v;
            }
        }
    });
}

// The inverse: staged frame j (feat / gmm / x_d3 planes, each optional) goes to slot slots[j] of the pool.  An entry outside
// [0, n_slots) skips the frame: its chunks store nothing.
__global__ __launch_bounds__(POOL_THREADS) void scatter_frames_kernel(const MagnetScatterFramesArgs a, const ChunkPlan<N_SC> p) {
    const int n = a.n;
    const int es = a.feat_dtype == MAGNET_FEAT_BF16 ? 2 : 4;
    const int R = (a.h + 2) * (a.w + 2);                              // rows of one padded frame
    walk_chunks(p, [&](int seg, int e, int u0, int u1, int units) {
        const bool lo = seg == SC_XD3 && e >= n;                      // x_d3 frames [0, n) = hi plane, [n, 2n) = lo plane
        const int j = lo ? e - n : e;                                 // staged frame
        const int slot = a.slots[j];
        if (slot < 0 || slot >= a.n_slots) return;                    // uniform over the chunk
        const size_t s = (size_t)slot;
        if (seg == SC_GMM) {
            const int len = 2 * a.h * a.w;
            const float* src = a.gmm + (size_t)j * len;
            float* dst = a.pool_gmm + s * len;
            for (int u = u0 + threadIdx.x; u < u1; u += POOL_THREADS) copy_gmm_unit(src, dst, len, u, false);
            return;
        }
        const size_t frame = seg == SC_FEAT ? (size_t)R * a.F * es : (size_t)R * 512;    // bytes = units * 16
        const char* src = static_cast<const char*>(seg == SC_FEAT ? a.feat : lo ? a.xd3_lo : a.xd3_hi) + (size_t)j * frame;
        char* dst = static_cast<char*>(seg == SC_FEAT ? a.pool_feat : lo ? a.pool_xd3_lo : a.pool_xd3_hi) + s * frame;
        for (int u = u0 + threadIdx.x; u < u1; u += POOL_THREADS)
            *reinterpret_cast<uint4*>(dst + (size_t)u * 16) = *reinterpret_cast<const uint4*>(src + (size_t)u * 16);
    });
}

}  // namespace

// The caller (api.hip) has checked the arguments: dimensions positive, F % 8 == 0, units of a frame below 2^31.
hipError_t launch_gather_views(const MagnetGatherViewsArgs& a, hipStream_t s) {
    const int es = a.feat_dtype == MAGNET_FEAT_BF16 ? 2 : 4;
    const long long R = (long long)(a.h + 2) * (a.w + 2);
    const long long VB = (long long)a.V * a.B;
    const long long units[N_SEG] = {(long long)a.h * a.w * a.F * es / 16, R * a.F * es / 16, 1 + ((long long)2 * a.h * a.w + 3) / 4,
                                    1 + ((long long)2 * a.h * a.w + 3) / 4, R * 32};
    const long long frames[N_SEG] = {a.ref_cl ? a.B : 0, a.src_pad ? VB : 0, a.ref_gmm ? a.B : 0, a.src_gmm ? VB : 0,
                                     a.gin_hi ? 2LL * a.B : 0};
    ChunkPlan<N_SEG> p;
    const long long total = plan_chunks(p, units, frames);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_views_kernel, dim3(chunk_grid(total)), dim3(POOL_THREADS), 0, s, a, p);
    return hipGetLastError();
}

// As above: api.hip has checked the arguments.
hipError_t launch_scatter_frames(const MagnetScatterFramesArgs& a, hipStream_t s) {
    const int es = a.feat_dtype == MAGNET_FEAT_BF16 ? 2 : 4;
    const long long R = (long long)(a.h + 2) * (a.w + 2);
    const long long units[N_SC] = {R * a.F * es / 16, 1 + ((long long)2 * a.h * a.w + 3) / 4, R * 32};
    const long long frames[N_SC] = {a.feat ? a.n : 0, a.gmm ? a.n : 0, a.xd3_hi ? 2LL * a.n : 0};
    ChunkPlan<N_SC> p;
    const long long total = plan_chunks(p, units, frames);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_frames_kernel, dim3(chunk_grid(total)), dim3(POOL_THREADS), 0, s, a, p);
    return hipGetLastError();
}

}  // namespace magnet
