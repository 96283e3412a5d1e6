// image_prep.hip — magnet_image_prep_u8: N raw camera frames, uint8 channel-last, to the (N, 3, Hout, Wout) fp32 tensor the
// backbones read, in one launch: integer crop, Pillow's 8-bit BILINEAR resize (Image.resize: a separable triangle filter whose
// support grows with the downscale ratio, in integer arithmetic) and the loader's normalisation as a table lookup.
// magnet_train_prep_u8 is the same body with a record per frame (lut_index, flip, win_x, win_y): the output is a window of the
// horizontally flipped resized image, looked up in that frame's own table (the sample's augmentation and the normalisation).
//
// A workgroup owns an IP_TW x IP_TH tile of the output.  It
//   1. copies the tile's coefficient rows and the 3 x 256 normalisation table into LDS,
//   2. stages, in LDS as uint8, the horizontal-pass results of the source rows its tile's vertical windows cover
//      (rows [bounds_y[first].xmin, bounds_y[last].xmin + n) of the crop box; the tile's own rows when the vertical pass is skipped),
//   3. runs the vertical pass from LDS, looks the 8-bit result up and stores the three channel planes, consecutive threads on
//      consecutive x.
// Both passes are   ss = (1 << 21) + sum_k coef[k] * pixel[xmin + k];  out = clamp(ss >> 22, 0, 255)   in int32 (the coefficients of
// a row sum to 2^22, so ss < 2^31).  A pass whose output size equals its input size is a copy, as in Pillow.  No floating-point
// arithmetic happens here: the fp32 values come from the caller's table.
//
// Bounds: the tables live in device memory and are not trusted.  Every window start is clamped into the crop box and every tap count
// to the row length and to what is left of the box, so no byte outside the crop box is read whatever the tables hold; the staged row
// count is clamped to IP_MAX_ROWS and every staged-row index to the rows staged.  With the tables of ingest.resample_tables none of
// the clamps acts.  The frame records are not trusted either: the table index, the flip and the window origin are clamped to their
// ranges, so every resized column and row a tile asks for exists in the tables.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/magnet_hip.h"

namespace magnet {

namespace {

constexpr int IP_TW = 80;                  // output columns of a tile: 320-byte store segments per row and plane
constexpr int IP_TH = 10;                  // output rows of a tile
constexpr int IP_THREADS = 256;
constexpr int IP_KMAX = MAGNET_IMAGE_PREP_KMAX;
// source rows under IP_TH output rows at the limit (scale = support = (IP_KMAX - 1) / 2): the first and the last window start
// (IP_TH - 1) * scale apart, the last one is 2 * support + 1 long at most, one more for the rounding of the first
constexpr int IP_MAX_ROWS = (IP_TH - 1) * ((IP_KMAX - 1) / 2) + (IP_KMAX - 1) + 2;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// What the two argument structs name differently: the size the tables are built for (the inference form's output is all of it).
__device__ __forceinline__ int res_h(const MagnetImagePrepArgs& a) { return a.Hout; }
__device__ __forceinline__ int res_w(const MagnetImagePrepArgs& a) { return a.Wout; }
__device__ __forceinline__ int res_h(const MagnetTrainPrepArgs& a) { return a.Hres; }
__device__ __forceinline__ int res_w(const MagnetTrainPrepArgs& a) { return a.Wres; }

// REC: the frame has a record.  Without one the window is the whole resized image, unflipped, and the table is a.lut: every
// expression on flip, wx, wy below folds away.
template <bool REC, class Args>
__device__ __forceinline__ void image_prep_body(const Args& a) {
    __shared__ uint8_t stage[IP_MAX_ROWS][3][IP_TW];
    __shared__ int32_t cx[IP_TW][IP_KMAX];
    __shared__ int32_t cy[IP_TH][IP_KMAX];
    __shared__ int32_t bx[IP_TW][2];
    __shared__ int32_t by[IP_TH][2];
    __shared__ float lut[3 * 256];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * IP_TW, y0 = blockIdx.y * IP_TH;
    const int tw = min(IP_TW, a.Wout - x0), th = min(IP_TH, a.Hout - y0);
    const int Hres = res_h(a), Wres = res_w(a);
    const bool horiz = a.crop_w != Wres, vert = a.crop_h != Hres;
    const int kx = a.kx, ky = a.ky;

    // the tile in the resized image: rows ry0 .. ascending, columns col(x), descending when the frame is flipped
    bool flip = false;
    int rx0 = x0, ry0 = y0;
    const float* table;
    if constexpr (REC) {
        const int32_t* rec = a.frame_params + 4 * (size_t)blockIdx.z;
        table = a.luts + (size_t)clampi(rec[0], 0, a.n_luts - 1) * (3 * 256);
        flip = rec[1] != 0;
        rx0 += clampi(rec[2], 0, Wres - a.Wout);
        ry0 += clampi(rec[3], 0, Hres - a.Hout);
    } else {
        table = a.lut;
    }
    const auto col = [&](int x) { return flip ? Wres - 1 - (rx0 + x) : rx0 + x; };

    // ---- 1. the tile's tables ----
    for (int i = tid; i < 3 * 256; i += IP_THREADS) lut[i] = table[i];
    if (horiz) {
        for (int i = tid; i < tw * kx; i += IP_THREADS) { const int x = i / kx; cx[x][i - x * kx] = a.coef_x[(size_t)col(x) * kx + (i - x * kx)]; }
        for (int x = tid; x < tw; x += IP_THREADS) {
            const int lo = clampi(a.bounds_x[2 * col(x)], 0, a.crop_w - 1);
            bx[x][0] = lo;
            bx[x][1] = clampi(a.bounds_x[2 * col(x) + 1], 0, min(kx, a.crop_w - lo));
        }
    }
    int r0 = ry0, r1 = ry0 + th;           // source rows of the crop box this tile reads: uniform over the workgroup
    if (vert) {
        for (int i = tid; i < th * ky; i += IP_THREADS) { const int y = i / ky; cy[y][i - y * ky] = a.coef_y[(size_t)(ry0 + y) * ky + (i - y * ky)]; }
        const int last = ry0 + th - 1;
        r0 = clampi(a.bounds_y[2 * ry0], 0, a.crop_h - 1);
        r1 = clampi(a.bounds_y[2 * last] + a.bounds_y[2 * last + 1], r0 + 1, min(a.crop_h, r0 + IP_MAX_ROWS));
        for (int y = tid; y < th; y += IP_THREADS) {
            by[y][0] = a.bounds_y[2 * (ry0 + y)] - r0;                // first staged row of the window; clamped per tap below
            by[y][1] = clampi(a.bounds_y[2 * (ry0 + y) + 1], 0, ky);
        }
    }
    const int rows = r1 - r0;
    __syncthreads();

    // ---- 2. horizontal pass of rows [r0, r1) into LDS; the channel is the fastest index, so a wavefront reads one stretch of a row ----
    const uint8_t* src = a.src + (size_t)blockIdx.z * a.src_frame + (size_t)(a.crop_top + r0) * a.src_pitch + (size_t)a.crop_left * 3;
    const int per_row = tw * 3;
    for (int i = tid; i < rows * per_row; i += IP_THREADS) {
        const int row = i / per_row, rem = i - row * per_row;
        const int x = rem / 3, c = rem - x * 3;
        const uint8_t* p = src + (size_t)row * a.src_pitch + c;
        int v;
        if (horiz) {
            const int n = bx[x][1];
            p += bx[x][0] * 3;
            int ss = 1 << 21;
            for (int k = 0; k < n; ++k) ss += cx[x][k] * (int)p[k * 3];
            v = clampi(ss >> 22, 0, 255);
        } else {
            v = p[col(x) * 3];
        }
        stage[row][c][x] = (uint8_t)v;
    }
    __syncthreads();

    // ---- 3. vertical pass from LDS, lookup, store: x is the fastest index ----
    const size_t plane = (size_t)a.Hout * a.Wout;
    float* out = a.out + (size_t)blockIdx.z * 3 * plane + (size_t)y0 * a.Wout + x0;
    for (int i = tid; i < th * per_row; i += IP_THREADS) {
        const int y = i / per_row, rem = i - y * per_row;
        const int c = rem / tw, x = rem - c * tw;
        int v;
        if (vert) {
            const int first = by[y][0], n = by[y][1];
            int ss = 1 << 21;
            for (int k = 0; k < n; ++k) ss += cy[y][k] * (int)stage[clampi(first + k, 0, rows - 1)][c][x];
            v = clampi(ss >> 22, 0, 255);
        } else {
            v = stage[y][c][x];
        }
        out[c * plane + (size_t)y * a.Wout + x] = lut[c * 256 + v];
    }
}

__global__ __launch_bounds__(IP_THREADS) void image_prep_kernel(const MagnetImagePrepArgs a) { image_prep_body<false>(a); }
__global__ __launch_bounds__(IP_THREADS) void train_prep_kernel(const MagnetTrainPrepArgs a) { image_prep_body<true>(a); }

}  // namespace

// The caller (api.hip) has checked the arguments: the crop box inside the frame, pitches that hold a row and a frame, tap counts
// within IP_KMAX and equal to what the sizes imply (which bounds the staged rows by IP_MAX_ROWS), N within the grid's z range;
// for the training form also 1 <= Hout <= Hres, 1 <= Wout <= Wres and n_luts >= 1.
hipError_t launch_image_prep(const MagnetImagePrepArgs& a, hipStream_t s) {
    const dim3 grid((a.Wout + IP_TW - 1) / IP_TW, (a.Hout + IP_TH - 1) / IP_TH, a.N);
    hipLaunchKernelGGL(image_prep_kernel, grid, dim3(IP_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_train_prep(const MagnetTrainPrepArgs& a, hipStream_t s) {
    const dim3 grid((a.Wout + IP_TW - 1) / IP_TW, (a.Hout + IP_TH - 1) / IP_TH, a.N);
    hipLaunchKernelGGL(train_prep_kernel, grid, dim3(IP_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace magnet
