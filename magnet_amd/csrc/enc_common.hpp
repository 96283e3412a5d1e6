// enc_common.hpp — launch parameters of the EfficientNet encoder's kernels (enc_kernels.hip), shared with api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_common.hpp"

namespace magnet {

// a depthwise workgroup's tile of output pixels: the partial channel sums are one row of `part` per tile
constexpr int ENC_DW_TH = 8, ENC_DW_TW = 16;
inline long long enc_dw_parts(long long ho, long long wo) { return ((ho + ENC_DW_TH - 1) / ENC_DW_TH) * ((wo + ENC_DW_TW - 1) / ENC_DW_TW); }

struct EncDwParams {
    const uint16_t* in_hi; const uint16_t* in_lo;     // (N, hi+2, wi+2, in_ld) planes
    int in_ld, hi, wi, c_pad;
    const float* wgt;                                 // [k*k][c_pad], BatchNorm folded, zero in the pad lanes
    const float* bias;                                // [c_pad]
    int k, stride, pad_top, pad_left;
    uint16_t* out_hi; uint16_t* out_lo;               // (N, ho+2, wo+2, out_ld) planes: the interior is written
    int out_ld, ho, wo;
    float* part;                                      // (N, n_part, c_pad)
    int n_part;                                       // set by the launcher: enc_dw_parts(ho, wo)
};

// f16 (the `_f16` entry points): the grids are ONE fp16 plane each, at the hi pointers; the lo pointers are NULL and unused
hipError_t launch_enc_stem(const float*, const float*, const float*, uint16_t*, uint16_t*, int, int, int, bool f16, hipStream_t);
hipError_t launch_enc_dwconv(const EncDwParams&, int N, bool f16, hipStream_t);
hipError_t launch_enc_se_gate(const float*, int, long long, const float*, const float*, const float*, const float*, int, int, int, float*, int, hipStream_t);
hipError_t launch_enc_se_scale(const uint16_t*, const uint16_t*, int, const float*, int, int, int, int, uint16_t*, uint16_t*, int, bool f16, hipStream_t);

}  // namespace magnet
