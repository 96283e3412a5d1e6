// pack.hpp — launchers of pack.hip: the NCHW fp32 -> channel-last layout packs and the planes -> fp16 conversion (api.hip calls them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace magnet {

// fp32 NCHW (N, C, h, w), images `in_img_stride` floats apart -> channels [c_off, c_off + C) of the interior of a channel-last buffer
// (N, h + 2, w + 2, ctot); launch_pack: (N, h + 2 pad, w + 2 pad, F), whose border it zeroes first when pad = 1
hipError_t launch_pack(const float* in, void* out, int N, int F, int h, int w, bool bf16, int pad, hipStream_t s);
hipError_t launch_pack_split(const float* in, uint16_t* out_hi, uint16_t* out_lo, int N, int C, int h, int w, int ctot, int c_off,
                             long long in_img_stride, hipStream_t s);
hipError_t launch_pack_f16(const float* in, uint16_t* out, int N, int C, int h, int w, int ctot, int c_off, long long in_img_stride,
                           hipStream_t s);
hipError_t launch_planes_to_f16(const uint16_t* in_hi, const uint16_t* in_lo, uint16_t* out, long long rows, int ld, int ld16, int c0, int c1,
                                hipStream_t s);

}  // namespace magnet
