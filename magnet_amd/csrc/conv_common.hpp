// conv_common.hpp — launch parameters of the matrix-core convolution kernels (conv_mfma.hip), shared with api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace magnet {

struct ConvParams {
    const uint16_t* in_hi;  const uint16_t* in_lo;    // activations, row 0 of the flattened padded grid (the fp16 routes: in_hi / w_hi
                                                      // are fp16 planes, in_lo / w_lo NULL)
    const uint16_t* w_hi;   const uint16_t* w_lo;     // [taps][cout_pad][cin]
    const float*    bias;                             // [cout_pad]
    uint16_t* out_hi; uint16_t* out_lo;               // OUT mode 0: bf16 planes [rows][cout_pad]
    float*    out_f32;                                // OUT mode 1: fp32 [rows][cout_pad]
    long long rows;                                   // B*(h+2)*(w+2)
    int cin, cout_pad, taps, wp, relu, out_mode;
    int in_ld;                                        // elements between consecutive input rows (>= cin)
    const float* addend;                              // optional fp32 (rows, addend_ld) added before bias/ReLU
    int addend_ld;
    int tap_off[9];                                   // input row offset of each tap (dilation / 2x2 windows: host-computed)
    int min_off, max_off;                             // min / max of tap_off[0..taps)
    int tap_n, tap_o0, tap_sy, tap_sx;                // taps = tap_n^2; offset of tap (ty,tx) = (ty+o0)*sy + (tx+o0)*sx — the kernel
                                                      // steps (ty,tx) with scalar counters instead of loading tap_off[] per K step
    int out_ld;                                       // elements between consecutive output rows (>= cout_pad)
    const uint16_t* add_hi; const uint16_t* add_lo;   // optional split-bf16 addend (residual connections), rows x add_ld
    int add_ld;
    int img_rows, hp, pad;                            // img_rows = hp*wp > 0: rows are decoded to (image, y, x) and outputs of
                                                      // the `pad`-wide border are written as zeros (next layer's zero padding)
    int repad;                                        // > 0: interior rows only, re-addressed to a grid with border repad-1
    // fused 1x1 tail (cout_pad == 128 only): relu(1x1 128->128), relu(1x1 128->128), 1x1 128->tail_cout applied to the
    // workgroup's tile before it leaves the CU; weights [128][128],[128][128],[tail_cout][128] concatenated, bias likewise
    const uint16_t* tail_w_hi; const uint16_t* tail_w_lo; const float* tail_bias;
    int tail_cout;                                    // 16, 128 or 144; result fp32 (rows, tail_cout) at out_f32
    // fused convex upsampling (tail_cout == 144 only; models/MAGNET.py:15-27): the tail's last layer keeps its (rows, 144) mask
    // logits in registers, soft-maxes the 9 neighbour weights of each of the 16 sub-pixels and writes the x4-upsampled (mu, sigma)
    // of up_npred stacked predictions: depth (up_npred, B, 2, up_h, up_w) -> up_out (up_npred, B, 2, 4 up_h, 4 up_w); nothing is
    // written to out_f32.  Rows are positions of (B, up_h + 2, up_w + 2) grids (wp = up_w + 2).
    const float* up_depth; float* up_out;
    int up_npred, up_h, up_w, up_B;
    // fused Gaussian update (tail_cout == 16 only; models/MAGNET.py:60-69): the G-Net head's two outputs (o0, o1) of an interior
    // position update (mu, sigma) in place of the (rows, 16) fp32 write: gu_in (up_B, 2, up_h, up_w) -> gu_out, same layout
    const float* gu_in; float* gu_out;
    int variant;                                      // host side only (launch_conv_mfma): 0; the dev library sets it from MAGNET_CONV_VARIANT
    // LeakyReLU (magnet_conv_mfma_ex; the D-Net decoder, D_dense_depth.py:29-43): leaky == 1 and relu == 0 -> negative outputs are
    // multiplied by leaky_slope after bias / addend.  Plain epilogue only (not with the fused tail)
    // leaky == 2: SiLU (MAGNET_ACT_SILU, magnet_conv_mfma_ex only; the EfficientNet encoder's expand layers): x * sigmoid(x) in the same
    // place (silu_f32 below)
    int leaky;
    float leaky_slope;
    // row tiling (launch_conv_mfma decides; see conv_mfma_tile).  tiles_per_img = 0: tile t starts at row t * BM of the flat buffer.
    // tiles_per_img > 0 (launches that carry up_B / up_h / wp): every image is tiled on its own from its first interior image row,
    // tile t starts at row (t / tiles_per_img) * (up_h + 2) * wp + wp + (t % tiles_per_img) * BM; the border image rows get no tile
    int tiles_per_img;
    int tiling;                                       // host side only: MAGNET_TILING_* of MagnetConvExArgs (0 = the launcher chooses)
    long long* tiles_out;                             // host side only, optional: receives the number of row tiles launched
};

// Row tiles of a launch over `n_img` zero-bordered (h + 2, wp) grids with `bm`-row tiles.  Returns the tile count and sets *per_img to
// the tiles per image (per-image tiling) or to 0 (flat tiling).  Per-image tiling covers the h * wp rows from each image's first
// interior image row; it is taken only when it launches FEWER tiles than the flat form and the last tile of an image ends inside that
// image (so a tile never computes rows of two images and every interior row belongs to exactly one tile).
inline long long conv_row_tiles(long long n_img, long long h, long long wp, long long bm, int* per_img) {
    const long long flat = (n_img * (h + 2) * wp + bm - 1) / bm, per = (h * wp + bm - 1) / bm;
    const bool by_image = n_img * per < flat && per * bm <= (h + 1) * wp;
    *per_img = by_image ? (int)per : 0;
    return by_image ? n_img * per : flat;
}

// fp32 -> fp16 bits as the single-plane fp16 format defines it (include/magnet_hip.h): round to nearest even, a magnitude that would
// round above 65504 (+-Inf included) becomes +-65504, NaN is written through, the sign of zero is kept.
// v_med3_f32 returns a finite bound for a NaN operand, so NaN bypasses the clamp; med3(-0, -65504, 65504) = -0
__device__ __forceinline__ uint32_t f16_bits_sat(float x) {
    const float c = x != x ? x : __builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f);
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)c);               // v_cvt_f16_f32: RNE, fp16 denormals kept
}
__device__ __forceinline__ uint32_t f16x2_bits_sat(float a, float b) { return f16_bits_sat(a) | (f16_bits_sat(b) << 16); }
// 8 fp32 -> one 16-byte vector of fp16 (f16_bits_sat each), and back (exact)
__device__ __forceinline__ uint4 f16x8_pack_sat(const float* v) {
    return make_uint4(f16x2_bits_sat(v[0], v[1]), f16x2_bits_sat(v[2], v[3]), f16x2_bits_sat(v[4], v[5]), f16x2_bits_sat(v[6], v[7]));
}
__device__ __forceinline__ void f16x8_unpack(const uint4 u, float* v) {
    typedef __attribute__((ext_vector_type(8))) _Float16 h8_t;
    const h8_t h = __builtin_bit_cast(h8_t, u);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
}

// sigmoid(x) = 1 / (1 + e), e = 2^(-x log2 e) on the hardware exponential (v_exp_f32: 1 ulp; the rounding of its argument and of the constant add a
// relative 1.3 |x| 2^-24 to e), one fp32 add and one correctly rounded divide; silu(x) = x / (1 + e).  e overflows to +Inf below x = -88.7 (result
// -0 for silu, +0 for sigmoid) and flushes to 0 above x = 87.3 (result x, 1): both within the bound.  Accuracy, stated for the tests
// (include/magnet_hip.h): |sigmoid_f32(x) - sigmoid(x)| <= 2^-21, |silu_f32(x) - silu(x)| <= 2^-21 |silu(x)| + 2^-22.
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + __builtin_amdgcn_exp2f(-x * 1.44269504088896341f)); }
__device__ __forceinline__ float silu_f32(float x) { return x / (1.0f + __builtin_amdgcn_exp2f(-x * 1.44269504088896341f)); }

// The route of a convolution launch: the operand format and what it serves.  CONV_BF16X3: (hi, lo) planes:
// magnet_conv_mfma and magnet_conv_mfma_ex.  CONV_F16: the single-plane fp16 operand format (magnet_conv_mfma_f16, which has checked
// what that format serves): no lo planes.  CONV_F16P: the same operands, plane to plane (magnet_conv_mfma_f16p): the residual is ONE
// fp16 plane (add_lo NULL) and out_mode 3 (one fp16 plane at out_hi) exists.  CONV_F16D: plane to plane, wide (magnet_conv_mfma_f16d,
// the D-Net decoder's plain layers, cout_pad % 128 == 0, LeakyReLU): no residual; out_mode 0, 1 or 3.  CONV_F16E: plane to plane, the
// EfficientNet encoder's 1x1 layers (magnet_conv_mfma_f16e): taps 1, SiLU, the fp16 residual plane, out_mode 3 or 1; cout_pad 32 / 64 on
// CONV_F16P's windowless instances, cout_pad % 128 == 0 on CONV_F16D's — no kernel instance of its own
enum ConvRoute { CONV_BF16X3, CONV_F16, CONV_F16P, CONV_F16D, CONV_F16E };

// magnet_conv_mfma_nchw: input channels [c0, cin) of the launch are read from ptr, (up_B, cin - c0, up_h, up_w) fp32, and split to
// (hi, lo) in LDS; the planes hold channels [0, c0) only (in_hi / in_lo may be NULL when c0 == 0).  Kernel arguments of the two
// fp32-source instances alone, so ConvParams — every other instance's argument block — is what it was
struct ConvSrc { const float* ptr; int c0; };

// One convolution launch on `route`.  split_k = 0: the plain launch.  split_k = S in 2 .. 8 (CONV_BF16X3 and CONV_F16D: magnet_conv_mfma_splitk,
// magnet_conv_mfma_f16d_splitk): split-K over S input-channel ranges, the partials into work (S x rows x cout_pad fp32), then the
// fixed-order reduce + epilogue launch.  hipErrorInvalidValue for a (route, split_k) pair or a form that has no kernel instance
// nchw != NULL (CONV_BF16X3, split_k = 0 only): the fp32-source form of the 256-row fused-tail launches
hipError_t launch_conv(const ConvParams&, ConvRoute route, int split_k, float* work, hipStream_t, const ConvSrc* nchw = nullptr);

}  // namespace magnet
