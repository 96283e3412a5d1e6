// depth_prep.hip — magnet_depth_prep_u16: N uint16 depth maps to the (N, 1, Hout, Wout) fp32 ground truth of a training sample, in one
// launch: integer crop, Pillow's NEAREST resize as an index table per axis (ingest.nearest_table), the frame's horizontal flip and crop
// window (the record magnet_train_prep_u8 reads), the sensor's "no measurement" code, and the loader's division.
//
// One thread per output element, consecutive threads on consecutive x: the stores are dense, the loads a gather along one source row.
// The division is the one floating-point operation, a correctly rounded fp32 division of an integer below 2^16 (exact in fp32) by the
// caller's divisor: numpy's `x.astype(float32) / 1000.0` to the bit (the build passes -fhip-fp32-correctly-rounded-divide-sqrt).
//
// Bounds: the index tables and the records live in device memory and are not trusted.  Every table entry is clamped into the crop box,
// the window origin into [0, Wres - Wout] x [0, Hres - Hout]; with the tables of ingest.nearest_table no clamp acts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"

namespace magnet {

namespace {

constexpr int DP_THREADS = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(DP_THREADS) void depth_prep_kernel(const MagnetDepthPrepArgs a) {
    const int x = blockIdx.x * DP_THREADS + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= a.Wout) return;
    const int32_t* rec = a.frame_params + 4 * (size_t)n;
    const bool flip = rec[1] != 0;
    const int rx = clampi(rec[2], 0, a.Wres - a.Wout) + x;                       // column and row of the resized image
    const int ry = clampi(rec[3], 0, a.Hres - a.Hout) + y;
    const int cxr = flip ? a.Wres - 1 - rx : rx;
    const int sx = a.idx_x ? clampi(a.idx_x[cxr], 0, a.crop_w - 1) : cxr;        // column and row of the crop box
    const int sy = a.idx_y ? clampi(a.idx_y[ry], 0, a.crop_h - 1) : ry;
    const int v = a.src[(size_t)n * a.src_frame + (size_t)(a.crop_top + sy) * a.src_pitch + (a.crop_left + sx)];
    a.out[((size_t)n * a.Hout + y) * a.Wout + x] = __fdiv_rn(v == a.invalid_code ? 0.0f : (float)v, a.divisor);
}

}  // namespace

// The caller (api.hip) has checked the arguments: the crop box inside the frame, pitches that hold a row and a frame, 1 <= Hout <= Hres,
// 1 <= Wout <= Wres <= 32768, an index table exactly for an axis that is resized (the others have Wres == crop_w / Hres == crop_h),
// N and Hout within the grid's z and y ranges.
hipError_t launch_depth_prep(const MagnetDepthPrepArgs& a, hipStream_t s) {
    const dim3 grid((a.Wout + DP_THREADS - 1) / DP_THREADS, a.Hout, a.N);
    hipLaunchKernelGGL(depth_prep_kernel, grid, dim3(DP_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace magnet
