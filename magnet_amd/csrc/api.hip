// api.hip — the extern "C" boundary declared in include/magnet_hip.h.  Argument checking, error
// reporting, kernel selection.  No device allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <initializer_list>
#include "cv_common.hpp"
#include "conv_common.hpp"
#include "pack.hpp"
#include "enc_common.hpp"

namespace magnet {
hipError_t launch_pack_gmm(const float*, float*, int, int, int, hipStream_t);
hipError_t launch_pack_gmm_quad(const float*, float*, int, int, int, hipStream_t);
hipError_t launch_gaussian_update(const float*, const float*, float*, int, int, hipStream_t);
hipError_t launch_upsample(const float*, const float*, float*, int, int, int, int, int, hipStream_t);
hipError_t launch_gaussian_update_cl(const float*, int, const float*, float*, int, int, int, hipStream_t);
hipError_t launch_upsample_cl(const float*, const float*, int, float*, int, int, int, int, hipStream_t);
hipError_t launch_fnet_stem(const float*, const float*, const float*, uint16_t*, uint16_t*, int, int, int, hipStream_t);
hipError_t launch_space_to_depth(const uint16_t*, const uint16_t*, uint16_t*, uint16_t*, int, int, int, int, int, hipStream_t);
hipError_t launch_avgpool_cl(const uint16_t*, const uint16_t*, int, int, int, int, int, int, int, uint16_t*, uint16_t*, hipStream_t);
hipError_t launch_upsample_bilinear_cl(const float*, int, int, int, int, uint16_t*, uint16_t*, int, int, int, int, int, hipStream_t);
hipError_t launch_fnet_stem_f16(const float*, const float*, const float*, uint16_t*, int, int, int, hipStream_t);
hipError_t launch_space_to_depth_f16(const uint16_t*, uint16_t*, int, int, int, int, int, hipStream_t);
hipError_t launch_avgpool_cl_f16(const uint16_t*, int, int, int, int, int, int, int, uint16_t*, hipStream_t);
hipError_t launch_upsample_bilinear_cl_f16(const float*, int, int, int, int, uint16_t*, int, int, int, int, int, hipStream_t);
hipError_t launch_depth_metrics(const float*, const float*, double*, int, int, int, float, float, int, int, int, int, hipStream_t);
long long depth_metrics_workspace_bytes(int);
hipError_t launch_depth_metrics_ex(const MagnetDepthMetricsArgs&, hipStream_t);
hipError_t launch_make_rays(const double*, float*, int, int, int, hipStream_t);
hipError_t launch_relative_poses(const double*, const double*, float*, int32_t*, int, int, hipStream_t);
hipError_t launch_nll_forward(const MagnetNllArgs&, hipStream_t);
hipError_t launch_nll_backward(const MagnetNllArgs&, hipStream_t);
hipError_t launch_upsample_backward(const MagnetUpsampleBwdArgs&, hipStream_t);
hipError_t launch_head_dgrad(const MagnetHeadDgradArgs&, hipStream_t);
hipError_t launch_wgrad(const MagnetWgradArgs&, hipStream_t);
long long wgrad_workspace_bytes(const MagnetWgradArgs&);
hipError_t launch_fnet_stem_raw(const float*, const float*, float*, int, int, int, hipStream_t);
hipError_t launch_bn_train_stats(const MagnetBnTrainArgs&, hipStream_t);
hipError_t launch_bn_train_apply(const MagnetBnTrainArgs&, hipStream_t);
hipError_t launch_wgrad_ex(const MagnetWgradExArgs&, hipStream_t);
long long wgrad_ex_workspace_bytes(const MagnetWgradExArgs&);
hipError_t launch_bn_train_backward(const MagnetBnBwdArgs&, hipStream_t);
hipError_t launch_fnet_grad_pack(const float*, uint16_t*, uint16_t*, int, int, int, int, int, int, hipStream_t);
hipError_t launch_fnet_d2s_backward(const float*, float*, int, int, int, int, int, hipStream_t);
hipError_t launch_spp_upsample_backward(const MagnetSppBwdArgs&, hipStream_t);
hipError_t launch_spp_pool_backward(const MagnetSppBwdArgs&, hipStream_t);
hipError_t launch_fnet_stem_wgrad(const float*, const uint16_t*, const uint16_t*, float*, double*, int, int, int, hipStream_t);
hipError_t launch_dnet_gauss_head(const float*, int, int, int, int, int, float*, hipStream_t);
hipError_t launch_dnet_upsample_gauss(const float*, int, const float*, int, int, int, int, float*, hipStream_t);
hipError_t launch_fnet_loss_forward(const MagnetFnetLossArgs&, hipStream_t);
hipError_t launch_fnet_loss_backward(const MagnetFnetLossArgs&, hipStream_t);
hipError_t launch_bn_sync_moments(const MagnetBnTrainArgs&, double*, hipStream_t);
hipError_t launch_bn_sync_merge(const MagnetBnTrainArgs&, const double*, int, double*, hipStream_t);
hipError_t launch_bn_sync_backward_sums(const MagnetBnBwdArgs&, double*, hipStream_t);
hipError_t launch_bn_sync_backward_apply(const MagnetBnBwdArgs&, const double*, int, const double*, hipStream_t);
long long dnet_loss_workspace_bytes(const MagnetDnetLossArgs&);
hipError_t launch_dnet_loss_forward(const MagnetDnetLossArgs&, hipStream_t);
hipError_t launch_dnet_loss_backward(const MagnetDnetLossArgs&, hipStream_t);
hipError_t launch_dnet_nll_forward(const MagnetDnetNllArgs&, hipStream_t);
hipError_t launch_dnet_nll_backward(const MagnetDnetNllArgs&, hipStream_t);
hipError_t launch_gather_views(const MagnetGatherViewsArgs&, hipStream_t);
hipError_t launch_scatter_frames(const MagnetScatterFramesArgs&, hipStream_t);
hipError_t launch_image_prep(const MagnetImagePrepArgs&, hipStream_t);
hipError_t launch_train_prep(const MagnetTrainPrepArgs&, hipStream_t);
hipError_t launch_depth_prep(const MagnetDepthPrepArgs&, hipStream_t);
}

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int hip_fail(hipError_t e, const char* what) {
    return fail(-(int)e, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" {

MAGNET_API int magnet_version(void) { return MAGNET_HIP_VERSION; }

MAGNET_API const char* magnet_last_error(void) { return g_err; }

MAGNET_API int magnet_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

MAGNET_API int magnet_pack_features(const float* nchw, void* out_cl, int32_t N, int32_t F, int32_t h, int32_t w,
                         int32_t out_dtype, int32_t pad, void* stream) {
    if (!nchw || !out_cl) return fail(MAGNET_E_NULL, "magnet_pack_features: NULL pointer");
    if (N <= 0 || F <= 0 || h <= 0 || w <= 0 || (F % 8) != 0)
        return fail(MAGNET_E_DIM, "magnet_pack_features: bad dims N=%d F=%d h=%d w=%d (F must be a multiple of 8)", N, F, h, w);
    if (out_dtype != MAGNET_FEAT_F32 && out_dtype != MAGNET_FEAT_BF16)
        return fail(MAGNET_E_DTYPE, "magnet_pack_features: unknown dtype %d", out_dtype);
    if (pad != 0 && pad != 1) return fail(MAGNET_E_DIM, "magnet_pack_features: pad must be 0 or 1");
    if (!aligned16(out_cl)) return fail(MAGNET_E_ALIGN, "magnet_pack_features: out_cl not 16-byte aligned");
    hipError_t e = magnet::launch_pack(nchw, out_cl, N, F, h, w, out_dtype == MAGNET_FEAT_BF16, pad, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_pack_features launch");
}

MAGNET_API int magnet_pack_gmm(const float* gmm_nchw, float* out_pad, int32_t N, int32_t h, int32_t w, void* stream) {
    if (!gmm_nchw || !out_pad) return fail(MAGNET_E_NULL, "magnet_pack_gmm: NULL pointer");
    if (N <= 0 || h <= 0 || w <= 0) return fail(MAGNET_E_DIM, "magnet_pack_gmm: bad dims N=%d h=%d w=%d", N, h, w);
    hipError_t e = magnet::launch_pack_gmm(gmm_nchw, out_pad, N, h, w, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_pack_gmm launch");
}

MAGNET_API int magnet_pack_gmm_quad(const float* gmm_nchw, float* out_quad, int32_t N, int32_t h, int32_t w, void* stream) {
    if (!gmm_nchw || !out_quad) return fail(MAGNET_E_NULL, "magnet_pack_gmm_quad: NULL pointer");
    if (N <= 0 || h <= 0 || w <= 0) return fail(MAGNET_E_DIM, "magnet_pack_gmm_quad: bad dims N=%d h=%d w=%d", N, h, w);
    if (!aligned16(out_quad)) return fail(MAGNET_E_ALIGN, "magnet_pack_gmm_quad: out_quad not 16-byte aligned");
    hipError_t e = magnet::launch_pack_gmm_quad(gmm_nchw, out_quad, N, h, w, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_pack_gmm_quad launch");
}

// argument checks + launch parameters shared by the matcher and the backward of its mode 1
static int cv_prepare(const MagnetCostVolumeArgs* a, magnet::CvParams& p, bool backward) {
    if (!a) return fail(MAGNET_E_NULL, "magnet_cost_volume_cw: args is NULL");
    if (!a->ref_feat_cl || !a->src_feat_pad || (!a->src_gmm_pad && !a->src_gmm_quad && a->mode != 1) || !a->poses || !a->is_valid || !a->intM ||
        (!a->rays && !a->ray_params) || (!backward && !a->cost && !a->cost_hi))
        return fail(MAGNET_E_NULL, "magnet_cost_volume_cw: a required pointer is NULL");
    if (!a->rays && (backward || a->path == 3))
        return fail(MAGNET_E_NULL, "magnet_cost_volume_cw: this kernel reads the ray table (ray_params alone serves path 0/1/2/4 forward): "
                                   "build it with magnet_make_rays");
    if (a->mode != 0 && a->mode != 1) return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: unknown mode %d", a->mode);
    if (a->mode == 1 && (!a->k_list || a->d_volume))
        return fail(MAGNET_E_NULL, "magnet_cost_volume_cw: mode 1 takes its depth bins from k_list (d_volume must be NULL)");
    if (a->mode == 1 && a->path == 3)
        return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: mode 1 is not implemented in the worklist kernel");
    if (a->mode == 0 && !a->d_volume && (!a->ref_gmm || !a->k_list))
        return fail(MAGNET_E_NULL, "magnet_cost_volume_cw: d_volume is NULL, so ref_gmm and k_list are required");
    if (a->B <= 0 || a->V <= 0 || a->F <= 0 || a->D <= 0 || a->h <= 0 || a->w <= 0)
        return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: non-positive dimension");
    if (a->D > MAGNET_MAX_CANDIDATES)
        return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: D=%d exceeds MAGNET_MAX_CANDIDATES=%d", a->D, MAGNET_MAX_CANDIDATES);
    if ((a->F % 8) != 0) return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: F=%d must be a multiple of 8", a->F);
    if (a->feat_dtype != MAGNET_FEAT_F32 && a->feat_dtype != MAGNET_FEAT_BF16)
        return fail(MAGNET_E_DTYPE, "magnet_cost_volume_cw: unknown feat_dtype %d", a->feat_dtype);
    if (a->src_gmm_quad && !aligned16(a->src_gmm_quad)) return fail(MAGNET_E_ALIGN, "magnet_cost_volume_cw: src_gmm_quad must be 16-byte aligned");
    if (!aligned16(a->ref_feat_cl) || !aligned16(a->src_feat_pad))
        return fail(MAGNET_E_ALIGN, "magnet_cost_volume_cw: feature pointers must be 16-byte aligned");
    if (a->V > 64) return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: V=%d exceeds 64 source views", a->V);
    if ((size_t)a->h * a->w * (size_t)a->F * (size_t)a->V * (size_t)a->B >= ((size_t)1 << 40))
        return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: problem too large");

    memset(&p, 0, sizeof(p));
    p.B = a->B; p.V = a->V; p.F = a->F; p.D = a->D; p.h = a->h; p.w = a->w;
    p.tiles_x = (a->w + magnet::TILE_W - 1) / magnet::TILE_W;
    p.tiles_y = (a->h + magnet::TILE_H - 1) / magnet::TILE_H;
    if ((size_t)p.tiles_x * p.tiles_y * (size_t)p.B >= 0x7fffffffu)
        return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: grid too large");
    p.feat_bf16 = (a->feat_dtype == MAGNET_FEAT_BF16);
    p.kappa = a->kappa;
#ifdef MAGNET_DEV
    p.ablate = (int)(a->dev_flags & 0xffffffu);                    // development switches: never in the product build
    { static const int forced = getenv("MAGNET_DEV_FLAGS") ? (int)strtol(getenv("MAGNET_DEV_FLAGS"), nullptr, 0) : 0; p.ablate |= forced; }   // dev: run the test-suite against a variant
#else
    p.ablate = 0;
#endif
    p.mode_f = a->mode;
    p.ref_feat = a->ref_feat_cl; p.src_feat = a->src_feat_pad; p.src_gmm = a->src_gmm_pad; p.src_gmq = a->src_gmm_quad;
    p.ref_gmm = a->ref_gmm; p.d_volume = a->d_volume; p.poses = a->poses; p.is_valid = a->is_valid;
    p.intM = a->intM; p.rays = a->rays; p.cost = a->cost; p.stats = a->stats;
    p.cost_hi = (uint16_t*)a->cost_hi; p.cost_lo = (uint16_t*)a->cost_lo; p.cost_ld = a->cost_ld;
    p.gate_bits = a->gate_bits;
    p.ray_params = a->rays ? nullptr : a->ray_params;           // the table wins when both are given
    if (a->cost_hi && (!a->cost_lo || a->cost_ld < a->D))
        return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: cost_hi needs cost_lo and cost_ld >= D");
    if (a->cost_hi && a->path != 0 && a->path != 2 && a->path != 4)
        return fail(MAGNET_E_SHAPE, "magnet_cost_volume_cw: the split channel-last output exists only in the candidate-lane kernels (path 0/2/4)");
    if (a->gate_bits && (a->path == 1 || a->path == 3 || a->mode != 0))
        return fail(MAGNET_E_SHAPE, "magnet_cost_volume_cw: gate_bits is written by the candidate-lane kernels only (path 0/2/4, mode 0)");
    p.cost_bstride = a->cost_batch_stride ? a->cost_batch_stride : (long long)a->D * a->h * a->w;
    if (p.cost_bstride < (long long)a->D * a->h * a->w)
        return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: cost_batch_stride smaller than D*h*w");
    if (!a->d_volume)
        for (int j = 0; j < a->D; ++j) p.k[j] = (float)a->k_list[j];     // MAGNET.py:155: fp32 scalar multiply
    return 0;
}

MAGNET_API int magnet_cost_volume_cw(const MagnetCostVolumeArgs* a, void* stream) {
    magnet::CvParams p;
    if (const int rc = cv_prepare(a, p, false)) return rc;
    hipError_t e = hipSuccess;
    bool handled = false;
    const int path = a->path;
    if (path < 0 || path > 4) return fail(MAGNET_E_DIM, "magnet_cost_volume_cw: unknown path %d", path);
    if (path == 0 || path == 4) {
        e = magnet::launch_cv_fast(p, (hipStream_t)stream, &handled);
        if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_cw production-matcher launch");
        if (!handled && path == 4)
            return fail(MAGNET_E_SHAPE, "magnet_cost_volume_cw: the production matcher needs fused sampling (d_volume == NULL), mode 0, "
                                      "stats == NULL and F*sizeof(feature) <= 512");
    }
    if (!handled && !a->src_gmm_pad && a->mode != 1)      // only the quad-form (mu, sigma) map was given and the kernel that reads it does not take this call
        return fail(MAGNET_E_SHAPE, "magnet_cost_volume_cw: this shape / path reads src_gmm_pad (magnet_pack_gmm); src_gmm_quad alone serves the "
                                    "production matcher for D > 32 only");
    if (!handled && (path == 0 || path == 2)) {
        e = magnet::launch_cv_cand(p, (hipStream_t)stream, &handled);
        if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_cw candidate-lane launch");
        if (!handled && path == 2)
            return fail(MAGNET_E_SHAPE, "magnet_cost_volume_cw: the candidate-lane kernel does not take this shape");
    } else if (handled) {
    } else if (path == 3) {
        e = magnet::launch_cv_worklist(p, (hipStream_t)stream, &handled);
        if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_cw worklist launch");
        if (!handled)
            return fail(MAGNET_E_SHAPE, "magnet_cost_volume_cw: the worklist kernel does not take this shape (D > 128 or very wide F)");
    }
    if (!handled) {
        if (a->cost_hi || a->gate_bits) return fail(MAGNET_E_SHAPE, "magnet_cost_volume_cw: this shape falls back to the generic kernel, which has no split / gate-bit output");
        e = magnet::launch_cv_generic(p, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_cw generic launch");
    }
    return 0;
}

MAGNET_API int magnet_cost_volume_f_backward(const MagnetCostVolumeArgs* a, const float* grad_cost, float* grad_ref_cl,
                                             float* grad_src_pad, void* stream) {
    magnet::CvParams p;
    if (const int rc = cv_prepare(a, p, true)) return rc;
    if (a->mode != 1) return fail(MAGNET_E_DIM, "magnet_cost_volume_f_backward: only mode 1 (est_costvolume_F) is differentiable");
    if (a->feat_dtype != MAGNET_FEAT_F32) return fail(MAGNET_E_DTYPE, "magnet_cost_volume_f_backward: fp32 features required");
    if (!grad_cost || !grad_ref_cl || !grad_src_pad) return fail(MAGNET_E_NULL, "magnet_cost_volume_f_backward: NULL gradient pointer");
    if (!aligned16(grad_ref_cl) || !aligned16(grad_src_pad))
        return fail(MAGNET_E_ALIGN, "magnet_cost_volume_f_backward: gradient buffers must be 16-byte aligned");
    bool handled = false;
    hipError_t e = magnet::launch_cvf_bwd(p, grad_cost, grad_ref_cl, grad_src_pad, (hipStream_t)stream, &handled);
    if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_f_backward launch");
    if (!handled) return fail(MAGNET_E_DIM, "magnet_cost_volume_f_backward: shape not supported (V > 29; F > 128 unless F %% 32 == 0 and V <= 4; or image too large)");
    return 0;
}

MAGNET_API int magnet_make_rays(const double* ray_params, float* rays_out, int32_t B, int32_t h, int32_t w, void* stream) {
    if (!ray_params || !rays_out) return fail(MAGNET_E_NULL, "magnet_make_rays: NULL pointer");
    if (B <= 0 || h <= 0 || w <= 0) return fail(MAGNET_E_DIM, "magnet_make_rays: bad dims B=%d h=%d w=%d", B, h, w);
    hipError_t e = magnet::launch_make_rays(ray_params, rays_out, B, h, w, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_make_rays launch");
}

MAGNET_API int magnet_relative_poses(const double* ext_ref, const double* ext_nghbr, float* poses_out, int32_t* is_valid_out,
                                     int32_t B, int32_t V, void* stream) {
    if (!ext_ref || !ext_nghbr || !poses_out || !is_valid_out) return fail(MAGNET_E_NULL, "magnet_relative_poses: NULL pointer");
    if (B <= 0 || V <= 0) return fail(MAGNET_E_DIM, "magnet_relative_poses: bad dims B=%d V=%d", B, V);
    hipError_t e = magnet::launch_relative_poses(ext_ref, ext_nghbr, poses_out, is_valid_out, B, V, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_relative_poses launch");
}

MAGNET_API int64_t magnet_cost_volume_f_backward_workspace(const MagnetCostVolumeArgs* a) {
    magnet::CvParams p;
    if (cv_prepare(a, p, true)) return -1;
    return (int64_t)magnet::cvf_gather_workspace_bytes(p);
}

MAGNET_API int magnet_cost_volume_f_backward_ws(const MagnetCostVolumeArgs* a, const float* grad_cost, float* grad_ref_cl,
                                                float* grad_src_pad, void* workspace, int64_t workspace_bytes, void* stream) {
    magnet::CvParams p;
    if (const int rc = cv_prepare(a, p, true)) return rc;
    if (a->mode != 1) return fail(MAGNET_E_DIM, "magnet_cost_volume_f_backward_ws: only mode 1 (est_costvolume_F) is differentiable");
    if (a->feat_dtype != MAGNET_FEAT_F32) return fail(MAGNET_E_DTYPE, "magnet_cost_volume_f_backward_ws: fp32 features required");
    if (!grad_cost || !grad_ref_cl || !grad_src_pad) return fail(MAGNET_E_NULL, "magnet_cost_volume_f_backward_ws: NULL gradient pointer");
    if (!aligned16(grad_ref_cl) || !aligned16(grad_src_pad))
        return fail(MAGNET_E_ALIGN, "magnet_cost_volume_f_backward_ws: gradient buffers must be 16-byte aligned");
    bool ref_ok = false, src_ok = false;
    hipError_t e = magnet::launch_cvf_bwd_ref_only(p, grad_cost, grad_ref_cl, (hipStream_t)stream, &ref_ok);
    if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_f_backward_ws grad_ref launch");
    if (ref_ok && !(CV_DEV(p) & 0x30)) {
        e = magnet::launch_cvf_gather_src(p, grad_cost, grad_src_pad, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes,
                                          (hipStream_t)stream, &src_ok);
        if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_f_backward_ws grad_src launch");
    }
    if (ref_ok && src_ok) return 0;
    // shapes / workspace the gather path does not take: the scatter kernels (grad_src_pad must have been zeroed by the caller)
    bool handled = false;
    e = magnet::launch_cvf_bwd(p, grad_cost, grad_ref_cl, grad_src_pad, (hipStream_t)stream, &handled);
    if (e != hipSuccess) return hip_fail(e, "magnet_cost_volume_f_backward_ws launch");
    if (!handled) return fail(MAGNET_E_DIM, "magnet_cost_volume_f_backward_ws: shape not supported (V > 29; F > 128 unless F %% 32 == 0 and V <= 4; or image too large)");
    return 0;
}

MAGNET_API int magnet_gaussian_update(const float* gnet_out, const float* gmm_in, float* gmm_out, int32_t B, int32_t hw,
                           void* stream) {
    if (!gnet_out || !gmm_in || !gmm_out) return fail(MAGNET_E_NULL, "magnet_gaussian_update: NULL pointer");
    if (B <= 0 || hw <= 0) return fail(MAGNET_E_DIM, "magnet_gaussian_update: bad dims B=%d hw=%d", B, hw);
    hipError_t e = magnet::launch_gaussian_update(gnet_out, gmm_in, gmm_out, B, hw, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_gaussian_update launch");
}

MAGNET_API int magnet_upsample_depth(const float* depth, const float* mask, float* out, int32_t B, int32_t C, int32_t h,
                          int32_t w, int32_t k, void* stream) {
    if (!depth || !mask || !out) return fail(MAGNET_E_NULL, "magnet_upsample_depth: NULL pointer");
    if (B <= 0 || h <= 0 || w <= 0 || (C != 1 && C != 2) || (k != 1 && k != 2 && k != 4 && k != 8))
        return fail(MAGNET_E_DIM, "magnet_upsample_depth: bad dims B=%d C=%d h=%d w=%d k=%d (C in {1,2}, k in {1,2,4,8})", B, C, h, w, k);
    if (k == 4 && !aligned16(out)) return fail(MAGNET_E_ALIGN, "magnet_upsample_depth: out not 16-byte aligned");
    hipError_t e = magnet::launch_upsample(depth, mask, out, B, C, h, w, k, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_upsample_depth launch");
}

// Every convolution entry point ends here: the checks of the common fields, then the launch on `mode` (magnet::ConvRoute, conv_common.hpp).
// leaky: 1 selects LeakyReLU(leaky_slope) after bias, 2 SiLU (validated by the entry point)
// split_k >= 2 (the split-K entry points, which have checked what that form serves): the split-K launches with workspace `work`; else 0
using magnet::ConvRoute; using magnet::CONV_BF16X3; using magnet::CONV_F16; using magnet::CONV_F16P; using magnet::CONV_F16D; using magnet::CONV_F16E;
// src / src_c0 (magnet_conv_mfma_nchw, which has checked them): input channels [src_c0, cin) come from the NCHW fp32 tensor `src`
static int conv_mfma_run(const MagnetConvArgs* a, ConvRoute mode, int leaky, float leaky_slope, int tiling, int64_t* tiles_out, int split_k, float* work,
                         void* stream, const float* src = nullptr, int src_c0 = 0) {
    if (!a) return fail(MAGNET_E_NULL, "magnet_conv_mfma: args is NULL");
    const bool f16 = mode != CONV_BF16X3;
    const bool planes = !src || src_c0 > 0;                          // the launch reads the activation planes
    if ((planes && (!a->in_hi || (!f16 && !a->in_lo))) || !a->w_hi || (!f16 && !a->w_lo) || !a->bias) return fail(MAGNET_E_NULL, "magnet_conv_mfma: NULL input pointer");
    if (mode == CONV_F16E) {
        if (a->out_mode != 1 && a->out_mode != 3) return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16e: out_mode must be 1 or 3");
    } else
    if (mode == CONV_F16D) {
        if (a->out_mode != 0 && a->out_mode != 1 && a->out_mode != 3) return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16d: out_mode must be 0, 1 or 3");
    } else
    if (mode == CONV_F16P ? (a->out_mode < 1 || a->out_mode > 3) : (a->out_mode < 0 || a->out_mode > 2))
        return fail(MAGNET_E_DIM, mode == CONV_F16P ? "magnet_conv_mfma_f16p: out_mode must be 1, 2 or 3" : "magnet_conv_mfma: out_mode must be 0, 1 or 2");
    const bool tail = a->tail_w_hi != nullptr;
    if (tail) {
        if (!a->tail_w_lo || !a->tail_bias || (!a->out_f32 && !a->up_out && !a->gu_out)) return fail(MAGNET_E_NULL, "magnet_conv_mfma: fused tail needs tail_w_lo, tail_bias and out_f32 (or up_out / gu_out)");
        if (a->cout_pad != 128 || (a->tail_cout_pad != 16 && a->tail_cout_pad != 128 && a->tail_cout_pad != 144))
            return fail(MAGNET_E_DIM, "magnet_conv_mfma: fused tail needs cout_pad == 128 and tail_cout_pad in {16,128,144}");
        if (!aligned16(a->tail_w_hi) || !aligned16(a->tail_w_lo) || !aligned16(a->tail_bias) || !aligned16(a->out_f32))
            return fail(MAGNET_E_ALIGN, "magnet_conv_mfma: fused tail pointers must be 16-byte aligned");
        if (a->border_hp || a->repad || a->add_hi) return fail(MAGNET_E_DIM, "magnet_conv_mfma: fused tail excludes border / repad / residual input");
    }
    if (!tail && (a->out_mode == 0 ? (!a->out_hi || !a->out_lo) : (a->out_mode == 1 ? !a->out_f32 : !a->out_hi)))
        return fail(MAGNET_E_NULL, "magnet_conv_mfma: NULL output pointer");
    if (a->rows <= 0 || a->cin <= 0 || (a->cin % 32) != 0) return fail(MAGNET_E_DIM, "magnet_conv_mfma: rows > 0 and cin %% 32 == 0 required (cin=%d)", a->cin);
    if (a->taps != 1 && a->taps != 4 && a->taps != 9) return fail(MAGNET_E_DIM, "magnet_conv_mfma: taps must be 1, 4 or 9");
    if (a->taps != 1 && a->wp < 3) return fail(MAGNET_E_DIM, "magnet_conv_mfma: wp (row pitch of the bordered grid) missing");
    if (!((a->cout_pad > 0 && a->cout_pad % 128 == 0) || a->cout_pad == 144 || a->cout_pad == 16 || a->cout_pad == 32 || a->cout_pad == 64))
        return fail(MAGNET_E_DIM, "magnet_conv_mfma: cout_pad=%d unsupported (multiple of 128, or 144, 64, 32, 16)", a->cout_pad);
    if (!aligned16(a->in_hi) || !aligned16(a->in_lo) || !aligned16(a->w_hi) || !aligned16(a->w_lo) || !aligned16(a->bias) ||
        (!tail && (a->out_mode == 0 ? (!aligned16(a->out_hi) || !aligned16(a->out_lo)) : (a->out_mode == 1 ? !aligned16(a->out_f32) : !aligned16(a->out_hi)))))
        return fail(MAGNET_E_ALIGN, "magnet_conv_mfma: pointers must be 16-byte aligned");
    if (a->dil < 0 || a->dil > 8) return fail(MAGNET_E_DIM, "magnet_conv_mfma: dil=%d out of range", a->dil);
    magnet::ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in_hi = (const uint16_t*)a->in_hi; p.in_lo = (const uint16_t*)a->in_lo;
    p.w_hi = (const uint16_t*)a->w_hi; p.w_lo = (const uint16_t*)a->w_lo; p.bias = a->bias;
    p.out_hi = (uint16_t*)a->out_hi; p.out_lo = (uint16_t*)a->out_lo; p.out_f32 = a->out_f32;
    p.rows = a->rows; p.cin = a->cin; p.cout_pad = a->cout_pad; p.taps = a->taps; p.wp = a->wp;
    p.relu = a->relu; p.out_mode = a->out_mode;
    p.in_ld = a->in_ld ? a->in_ld : a->cin;
    p.addend = a->addend; p.addend_ld = a->addend_ld ? a->addend_ld : a->cout_pad;
    if (a->addend && (!aligned16(a->addend) || (p.addend_ld % 4) != 0 || p.addend_ld < a->cout_pad))
        return fail(MAGNET_E_ALIGN, "magnet_conv_mfma: addend must be 16-byte aligned with addend_ld >= cout_pad, a multiple of 4");
    if (p.in_ld < a->cin || (p.in_ld % 8) != 0) return fail(MAGNET_E_DIM, "magnet_conv_mfma: in_ld=%d must be >= cin and a multiple of 8", p.in_ld);
    const int dil = a->dil > 1 ? a->dil : 1;
    if (a->taps == 9) for (int t = 0; t < 9; ++t) p.tap_off[t] = ((t / 3 - 1) * a->wp + (t % 3 - 1)) * dil;
    if (a->taps == 4) { p.tap_off[0] = -a->wp - 1; p.tap_off[1] = -a->wp; p.tap_off[2] = -1; p.tap_off[3] = 0; }
    p.tap_n = a->taps == 9 ? 3 : (a->taps == 4 ? 2 : 1);
    p.tap_o0 = a->taps == 1 ? 0 : -1;
    p.tap_sy = a->taps == 9 ? a->wp * dil : (a->taps == 4 ? a->wp : 0);
    p.tap_sx = a->taps == 9 ? dil : (a->taps == 4 ? 1 : 0);
    for (int t = 0; t < a->taps; ++t) { p.min_off = p.tap_off[t] < p.min_off ? p.tap_off[t] : p.min_off; p.max_off = p.tap_off[t] > p.max_off ? p.tap_off[t] : p.max_off; }
    if (((long long)128 + p.max_off - p.min_off + 256) * (long long)p.in_ld * 2 >= ((long long)1 << 31) || (long long)a->taps * a->cout_pad * a->cin * 2 >= ((long long)1 << 31))
        return fail(MAGNET_E_DIM, "magnet_conv_mfma: row window or weight tensor exceeds 2 GiB");
    p.out_ld = a->out_ld ? a->out_ld : a->cout_pad;
    if (p.out_ld < a->cout_pad || (p.out_ld % 8) != 0) return fail(MAGNET_E_DIM, "magnet_conv_mfma: out_ld=%d must be >= cout_pad and a multiple of 8", p.out_ld);
    p.add_hi = (const uint16_t*)a->add_hi; p.add_lo = (const uint16_t*)a->add_lo; p.add_ld = a->add_ld ? a->add_ld : a->cout_pad;
    if (mode != CONV_F16P && mode != CONV_F16E && (a->add_hi != nullptr) != (a->add_lo != nullptr)) return fail(MAGNET_E_NULL, "magnet_conv_mfma: add_hi and add_lo come together");
    if (a->add_hi && (!aligned16(a->add_hi) || !aligned16(a->add_lo) || (p.add_ld % 8) != 0 || p.add_ld < a->cout_pad))
        return fail(MAGNET_E_ALIGN, "magnet_conv_mfma: add_hi/add_lo must be 16-byte aligned with add_ld >= cout_pad, a multiple of 8");
    // the epilogue holds ONE pre-bias term per channel: with both, the addend would replace the residual (no caller passes both)
    if (a->addend && a->add_hi) return fail(MAGNET_E_DIM, "magnet_conv_mfma: addend and add_hi/add_lo exclude each other (one pre-bias term per launch)");
    if (a->border_hp) {
        if (a->wp < 1 || a->border_pad < 0 || a->border_hp <= 2 * a->border_pad || a->wp <= 2 * a->border_pad ||
            (a->rows % ((long long)a->border_hp * a->wp)) != 0)
            return fail(MAGNET_E_DIM, "magnet_conv_mfma: border_hp=%d wp=%d border_pad=%d do not tile rows=%lld", a->border_hp, a->wp, a->border_pad, (long long)a->rows);
        if ((long long)a->border_hp * a->wp >= (1 << 24)) return fail(MAGNET_E_DIM, "magnet_conv_mfma: border_hp * wp must be < 2^24");
        p.img_rows = a->border_hp * a->wp; p.hp = a->border_hp; p.pad = a->border_pad;
    }
    if (a->repad < 0 || (a->repad && !a->border_hp)) return fail(MAGNET_E_DIM, "magnet_conv_mfma: repad needs border_hp");
    p.repad = a->repad;
    p.tail_w_hi = (const uint16_t*)a->tail_w_hi; p.tail_w_lo = (const uint16_t*)a->tail_w_lo; p.tail_bias = a->tail_bias;
    p.tail_cout = a->tail_cout_pad;
    if (a->up_out || a->up_depth) {                                  // fused convex upsampling in the tail's last layer
        if (!a->up_out || !a->up_depth) return fail(MAGNET_E_NULL, "magnet_conv_mfma: up_depth and up_out come together");
        if (!tail || a->tail_cout_pad != 144) return fail(MAGNET_E_DIM, "magnet_conv_mfma: the fused upsampling needs the 144-channel fused tail");
        if (a->up_npred <= 0 || a->up_B <= 0 || a->up_h <= 0 || a->up_w <= 0 || a->wp != a->up_w + 2 ||
            a->rows != (long long)a->up_B * (a->up_h + 2) * (a->up_w + 2) || a->rows >= ((long long)1 << 31))
            return fail(MAGNET_E_DIM, "magnet_conv_mfma: up_B=%d up_h=%d up_w=%d do not describe rows=%lld, wp=%d", a->up_B, a->up_h, a->up_w,
                        (long long)a->rows, a->wp);
        if (!aligned16(a->up_out) || ((uintptr_t)a->up_depth & 3)) return fail(MAGNET_E_ALIGN, "magnet_conv_mfma: up_out must be 16-byte aligned");
        p.up_depth = a->up_depth; p.up_out = a->up_out; p.up_npred = a->up_npred; p.up_B = a->up_B; p.up_h = a->up_h; p.up_w = a->up_w;
    }
    if (a->gu_out || a->gu_in) {                                     // fused Gaussian update behind G-Net's head
        if (!a->gu_out || !a->gu_in || a->gu_in == a->gu_out) return fail(MAGNET_E_NULL, "magnet_conv_mfma: gu_in and gu_out come together and must not alias");
        if (!tail || a->tail_cout_pad != 16 || a->up_out) return fail(MAGNET_E_DIM, "magnet_conv_mfma: the fused Gaussian update needs the 16-channel fused tail");
        if (a->up_B <= 0 || a->up_h <= 0 || a->up_w <= 0 || a->wp != a->up_w + 2 || a->rows != (long long)a->up_B * (a->up_h + 2) * (a->up_w + 2) ||
            a->rows >= ((long long)1 << 31))
            return fail(MAGNET_E_DIM, "magnet_conv_mfma: up_B=%d up_h=%d up_w=%d do not describe rows=%lld, wp=%d", a->up_B, a->up_h, a->up_w,
                        (long long)a->rows, a->wp);
        p.gu_in = a->gu_in; p.gu_out = a->gu_out; p.up_B = a->up_B; p.up_h = a->up_h; p.up_w = a->up_w;
    }
    p.leaky = leaky; p.leaky_slope = leaky_slope;
    long long tiles = 0;
    p.tiling = tiling; p.tiles_out = tiles_out ? &tiles : nullptr;
#ifdef MAGNET_DEV
    { static const int dev_variant = getenv("MAGNET_CONV_VARIANT") ? atoi(getenv("MAGNET_CONV_VARIANT")) : 0; p.variant = dev_variant; }   // dev A/B switch (dev build only)
#endif
    const magnet::ConvSrc nchw{src, src_c0};
    const hipError_t e = magnet::launch_conv(p, mode, split_k, work, (hipStream_t)stream, src ? &nchw : nullptr);
    if (tiles_out) *tiles_out = tiles;
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_conv_mfma launch");
}

// conv_mfma_run with the activation, tiling and tiles_out of an _ex argument struct (whose entry point has checked them)
static int conv_mfma_run(const MagnetConvExArgs* a, ConvRoute mode, int split_k, float* work, void* stream) {
    return conv_mfma_run(&a->base, mode, a->act == MAGNET_ACT_LEAKY_RELU ? 1 : (a->act == MAGNET_ACT_SILU ? 2 : 0), a->act_slope, a->tiling, a->tiles_out,
                         split_k, work, stream);
}

// The checks that several entry points (`who`) make, each stated once: 0, or the MAGNET_E_* code with the message set.
// The activation: act is known, LeakyReLU excludes relu (excludes_tail: and the fused tail) and takes a finite slope
// serves_silu: MAGNET_ACT_SILU is this entry point's (magnet_conv_mfma_ex alone): relu and the fused tail exclude it too
static int conv_act_check(const MagnetConvExArgs* a, const char* who, bool excludes_tail, bool serves_silu = false) {
    if (a->act == MAGNET_ACT_SILU) {
        if (!serves_silu) return fail(MAGNET_E_DIM, "%s: act=%d (MAGNET_ACT_SILU is served by magnet_conv_mfma_ex only)", who, a->act);
        if (a->base.relu || a->base.tail_w_hi) return fail(MAGNET_E_DIM, "%s: SiLU excludes relu and the fused tail", who);
        return 0;
    }
    if (a->act != MAGNET_ACT_BASE && a->act != MAGNET_ACT_LEAKY_RELU) return fail(MAGNET_E_DIM, "%s: act=%d unknown", who, a->act);
    if (a->act == MAGNET_ACT_LEAKY_RELU) {
        if (a->base.relu || (excludes_tail && a->base.tail_w_hi))
            return fail(MAGNET_E_DIM, excludes_tail ? "%s: LeakyReLU excludes relu and the fused tail" : "%s: LeakyReLU excludes relu", who);
        if (!(a->act_slope == a->act_slope) || a->act_slope > 1e30f || a->act_slope < -1e30f) return fail(MAGNET_E_DIM, "%s: act_slope must be finite", who);
    }
    return 0;
}

// The single-plane fp16 routes: planes of another format (bf16x3 lo planes) are refused rather than mis-read.
// res_planes: the residual planes the route takes.  1: ONE fp16 plane at add_hi (add_lo NULL); 0: no residual input (both NULL);
// 2: add_hi / add_lo are not this check's matter (magnet_conv_mfma_f16 refuses them with its border and repad forms)
static int conv_f16_planes_check(const MagnetConvArgs& b, const char* who, int res_planes) {
    if (b.in_lo || b.w_lo || (res_planes < 2 && b.add_lo) || (res_planes < 1 && b.add_hi))
        return fail(MAGNET_E_DIM, "%s: in_lo%s must be NULL (every operand is ONE fp16 plane)", who,
                    res_planes == 0 ? ", w_lo, add_hi and add_lo" : res_planes == 1 ? ", w_lo and add_lo" : " and w_lo");
    return 0;
}

// The plain layer on 128-row tiles only: no fused tail, addend, Gaussian update or upsampling; excludes_planes: no residual input either
static int conv_plain_check(const MagnetConvExArgs* a, const char* who, const char* format, bool excludes_planes) {
    const MagnetConvArgs& b = a->base;
    if (a->tiling & ~MAGNET_TILING_FLAT) return fail(MAGNET_E_DIM, "%s: tiling=%d (0 or MAGNET_TILING_FLAT: 128-row tiles only)", who, a->tiling);
    if (b.tail_w_hi || b.tail_w_lo || b.addend || b.up_out || b.up_depth || b.gu_in || b.gu_out ||
        (excludes_planes && (b.add_hi || b.add_lo)))
        return fail(MAGNET_E_DIM, "%s: the plain %s layer only (no fused tail, addend, %sGaussian update or upsampling)", who, format,
                    excludes_planes ? "residual input, " : "");
    return 0;
}

MAGNET_API int magnet_conv_mfma(const MagnetConvArgs* a, void* stream) { return conv_mfma_run(a, CONV_BF16X3, 0, 0.f, 0, nullptr, 0, nullptr, stream); }

MAGNET_API int magnet_conv_mfma_ex(const MagnetConvExArgs* a, void* stream) {
    if (!a) return fail(MAGNET_E_NULL, "magnet_conv_mfma_ex: args is NULL");
    if (const int rc = conv_act_check(a, "magnet_conv_mfma_ex", true, true)) return rc;
    if (a->tiling & ~(MAGNET_TILING_FLAT | MAGNET_TILING_BM256 | MAGNET_TILING_BM64)) return fail(MAGNET_E_DIM, "magnet_conv_mfma_ex: tiling=%d unknown", a->tiling);
    if (a->tiling & MAGNET_TILING_BM64) {                            // the 64-row instances: 3x3, 128-wide, bf16x3 operands
        const MagnetConvArgs& b = a->base;
        if (a->tiling & MAGNET_TILING_BM256) return fail(MAGNET_E_DIM, "magnet_conv_mfma_ex: MAGNET_TILING_BM64 and MAGNET_TILING_BM256 exclude each other");
        if (b.taps != 9 || (b.tail_w_hi ? b.cout_pad != 128 : (b.cout_pad <= 0 || b.cout_pad % 128 != 0)))
            return fail(MAGNET_E_DIM, "magnet_conv_mfma_ex: MAGNET_TILING_BM64 serves 3x3 launches (taps == 9) with cout_pad == 128 and a fused tail, or plain "
                                      "with cout_pad %% 128 == 0, bf16x3 operands only (taps=%d cout_pad=%d)", b.taps, b.cout_pad);
    }
    return conv_mfma_run(a, CONV_BF16X3, 0, nullptr, stream);
}

// The fused 3x3 launches of the 256-row kernel with x_d3 read in place: every refusal is made here, before conv_mfma_run's common checks
MAGNET_API int magnet_conv_mfma_nchw(const MagnetConvNchwArgs* a, void* stream) {
    const char* who = "magnet_conv_mfma_nchw";
    if (!a) return fail(MAGNET_E_NULL, "%s: args is NULL", who);
    const MagnetConvExArgs& x = a->ex;
    const MagnetConvArgs& b = x.base;
    if (!a->src) return fail(MAGNET_E_NULL, "%s: src is NULL", who);
    if (x.act != MAGNET_ACT_BASE) return fail(MAGNET_E_DIM, "%s: act=%d (MAGNET_ACT_BASE only)", who, x.act);
    if (x.tiling & ~MAGNET_TILING_BM256) return fail(MAGNET_E_DIM, "%s: tiling=%d (0 or MAGNET_TILING_BM256: per-image 256-row tiles only)", who, x.tiling);
    if (b.taps != 9 || b.dil > 1 || b.cout_pad != 128 || b.addend || b.add_hi || b.add_lo || b.border_hp || b.repad)
        return fail(MAGNET_E_DIM, "%s: bf16x3 3x3 layers (taps == 9, no dilation) with cout_pad == 128; no addend, residual, border or repad", who);
    if (!b.tail_w_hi || !((b.tail_cout_pad == 16 && b.gu_in && b.gu_out && !b.up_out && !b.up_depth) ||
                          (b.tail_cout_pad == 144 && b.up_depth && b.up_out && !b.gu_in && !b.gu_out)))
        return fail(MAGNET_E_DIM, "%s: the fused tail of 16 outputs with gu_in / gu_out, or of 144 outputs with up_depth / up_out", who);
    if (b.rows < 256ll * 256 && !(x.tiling & MAGNET_TILING_BM256))
        return fail(MAGNET_E_DIM, "%s: the 256-row kernel only (rows >= 65536 or MAGNET_TILING_BM256; rows=%lld)", who, (long long)b.rows);
    if (a->src_c0 < 0 || a->src_c0 % 32 || a->src_C <= 0 || a->src_C % 32 || (long long)a->src_c0 + a->src_C != b.cin)
        return fail(MAGNET_E_DIM, "%s: src_c0=%d and src_C=%d must be multiples of 32 with src_c0 + src_C == cin=%d", who, a->src_c0, a->src_C, b.cin);
    if (!aligned16(a->src)) return fail(MAGNET_E_ALIGN, "%s: src must be 16-byte aligned", who);
    if (b.up_B <= 0 || b.up_h <= 0 || b.up_w <= 0 || b.wp != b.up_w + 2 || b.rows != (long long)b.up_B * (b.up_h + 2) * (b.up_w + 2))
        return fail(MAGNET_E_DIM, "%s: up_B=%d up_h=%d up_w=%d do not describe rows=%lld, wp=%d", who, b.up_B, b.up_h, b.up_w, (long long)b.rows, b.wp);
    if ((long long)(b.up_h + 2) * b.wp >= (1 << 24) || (long long)a->src_C * b.up_h * b.up_w * 4 >= ((long long)1 << 31))
        return fail(MAGNET_E_DIM, "%s: an image of src exceeds 2 GiB, or its padded grid 2^24 positions", who);
    int per_img = 0;
    magnet::conv_row_tiles(b.up_B, b.up_h, b.wp, 256, &per_img);
    if (!per_img) return fail(MAGNET_E_DIM, "%s: per-image tiling is not in effect for %d images of %d x %d (flat tiling launches no more tiles)", who, b.up_B, b.up_h, b.up_w);
    return conv_mfma_run(&b, CONV_BF16X3, 0, 0.f, x.tiling, x.tiles_out, 0, nullptr, stream, a->src, a->src_c0);
}

MAGNET_API int magnet_conv_mfma_f16(const MagnetConvExArgs* a, void* stream) {
    if (!a) return fail(MAGNET_E_NULL, "magnet_conv_mfma_f16: args is NULL");
    const MagnetConvArgs& b = a->base;
    if (const int rc = conv_f16_planes_check(b, "magnet_conv_mfma_f16", 2)) return rc;
    if (a->act != MAGNET_ACT_BASE) return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16: act=%d (MAGNET_ACT_BASE only)", a->act);
    if (a->tiling & ~(MAGNET_TILING_FLAT | MAGNET_TILING_BM256))
        return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16: tiling=%d (MAGNET_TILING_FLAT and MAGNET_TILING_BM256 only)", a->tiling);
    if (b.taps != 9 || b.dil > 1 || b.cout_pad != 128)
        return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16: 3x3 layers (taps == 9, no dilation) with cout_pad == 128 only (taps=%d dil=%d cout_pad=%d)", b.taps, b.dil, b.cout_pad);
    if (b.add_hi || b.add_lo || b.border_hp || b.repad) return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16: no residual input, border or repad form");
    if (b.tail_w_hi ? (b.tail_cout_pad != 16 && b.tail_cout_pad != 144) : b.out_mode != 1)
        return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16: a fused tail of 16 or 144 outputs, or the plain layer with fp32 output (out_mode 1)");
    return conv_mfma_run(a, CONV_F16, 0, nullptr, stream);
}

MAGNET_API int magnet_conv_mfma_f16p(const MagnetConvExArgs* a, void* stream) {
    if (!a) return fail(MAGNET_E_NULL, "magnet_conv_mfma_f16p: args is NULL");
    const MagnetConvArgs& b = a->base;
    if (const int rc = conv_f16_planes_check(b, "magnet_conv_mfma_f16p", 1)) return rc;
    if (a->act != MAGNET_ACT_BASE) return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16p: act=%d (MAGNET_ACT_BASE only)", a->act);
    if (const int rc = conv_plain_check(a, "magnet_conv_mfma_f16p", "fp16", false)) return rc;
    if (b.cout_pad != 32 && b.cout_pad != 64 && b.cout_pad != 128) return fail(MAGNET_E_DIM, "magnet_conv_mfma_f16p: cout_pad=%d (32, 64 or 128)", b.cout_pad);
    return conv_mfma_run(a, CONV_F16P, 0, nullptr, stream);
}

// The EfficientNet encoder's 1x1 layers on fp16 planes: what magnet_conv_mfma_f16p (no SiLU) and magnet_conv_mfma_f16d (no SiLU, no
// residual) refuse, on their kernel instances.  Every refusal of the form is made here, under this entry point's name
MAGNET_API int magnet_conv_mfma_f16e(const MagnetConvExArgs* a, void* stream) {
    const char* who = "magnet_conv_mfma_f16e";
    if (!a) return fail(MAGNET_E_NULL, "%s: args is NULL", who);
    const MagnetConvArgs& b = a->base;
    if (const int rc = conv_f16_planes_check(b, who, 1)) return rc;
    if (a->act != MAGNET_ACT_BASE && a->act != MAGNET_ACT_SILU) return fail(MAGNET_E_DIM, "%s: act=%d (MAGNET_ACT_BASE or MAGNET_ACT_SILU)", who, a->act);
    if (b.relu) return fail(MAGNET_E_DIM, "%s: relu=%d (no ReLU: the layers are linear or SiLU)", who, b.relu);
    if (const int rc = conv_plain_check(a, who, "fp16", false)) return rc;
    if (b.taps != 1 || b.dil > 1) return fail(MAGNET_E_DIM, "%s: taps=%d dil=%d (1x1 layers only: taps == 1, no dilation)", who, b.taps, b.dil);
    if (b.cout_pad != 32 && b.cout_pad != 64 && (b.cout_pad <= 0 || b.cout_pad % 128 != 0))
        return fail(MAGNET_E_DIM, "%s: cout_pad=%d (32, 64 or a multiple of 128)", who, b.cout_pad);
    if (b.out_mode != 1 && b.out_mode != 3) return fail(MAGNET_E_DIM, "%s: out_mode=%d (3: one fp16 plane, 1: fp32)", who, b.out_mode);
    return conv_mfma_run(a, CONV_F16E, 0, nullptr, stream);
}

// What magnet_conv_mfma_f16d and its split-K form serve (`who`), before conv_mfma_run's checks of the common fields
static int conv_f16d_check(const MagnetConvExArgs* a, const char* who) {
    if (!a) return fail(MAGNET_E_NULL, "%s: args is NULL", who);
    const MagnetConvArgs& b = a->base;
    if (const int rc = conv_f16_planes_check(b, who, 0)) return rc;
    if (const int rc = conv_act_check(a, who, false)) return rc;
    if (const int rc = conv_plain_check(a, who, "fp16", false)) return rc;
    if ((b.taps != 1 && b.taps != 9) || b.dil > 1) return fail(MAGNET_E_DIM, "%s: taps=%d dil=%d (taps 1 or 9, no dilation)", who, b.taps, b.dil);
    if (b.cout_pad <= 0 || b.cout_pad % 128 != 0) return fail(MAGNET_E_DIM, "%s: cout_pad=%d must be a multiple of 128", who, b.cout_pad);
    if (b.out_mode != 0 && b.out_mode != 1 && b.out_mode != 3)
        return fail(MAGNET_E_DIM, "%s: out_mode=%d (0: split-bf16 planes, 1: fp32, 3: one fp16 plane)", who, b.out_mode);
    return 0;
}

// What the split-K form serves (both entry points and their workspace queries): 0, or the MAGNET_E_* code with the message set.
// *bytes: the workspace size.  f16d: the form on fp16 planes: conv_f16d_check first (out_mode 3 exists there), then the same limits
static const char* conv_splitk_who(bool f16d) { return f16d ? "magnet_conv_mfma_f16d_splitk" : "magnet_conv_mfma_splitk"; }
static int conv_splitk_check(const MagnetConvExArgs* a, int32_t split_k, int64_t* bytes, bool f16d) {
    const char* who = conv_splitk_who(f16d);
    if (f16d) { if (const int rc = conv_f16d_check(a, who)) return rc; }
    else if (!a) return fail(MAGNET_E_NULL, "%s: args is NULL", who);
    const MagnetConvArgs& b = a->base;
    if (split_k < 2 || split_k > MAGNET_SPLITK_MAX) return fail(MAGNET_E_DIM, "%s: split_k=%d (2 .. %d)", who, split_k, MAGNET_SPLITK_MAX);
    if (const int rc = conv_plain_check(a, who, f16d ? "fp16" : "bf16x3", true)) return rc;
    if (b.taps != 1 && b.taps != 9) return fail(MAGNET_E_DIM, "%s: taps=%d (1 or 9)", who, b.taps);
    if (b.cout_pad <= 0 || b.cout_pad % 128 != 0) return fail(MAGNET_E_DIM, "%s: cout_pad=%d must be a multiple of 128", who, b.cout_pad);
    if (!f16d && b.out_mode != 0 && b.out_mode != 1) return fail(MAGNET_E_DIM, "%s: out_mode=%d (0: split-bf16 planes, 1: fp32)", who, b.out_mode);
    if (b.rows <= 0 || b.cin <= 0 || (b.cin % 32) != 0) return fail(MAGNET_E_DIM, "%s: rows > 0 and cin %% 32 == 0 required (cin=%d)", who, b.cin);
    if ((b.cin / 32) / split_k < MAGNET_SPLITK_MIN_CHUNKS)
        return fail(MAGNET_E_DIM, "%s: cin=%d gives a split fewer than %d 32-channel chunks at split_k=%d", who, b.cin, MAGNET_SPLITK_MIN_CHUNKS, split_k);
    if (b.rows >= ((int64_t)1 << 31) || b.rows * (b.cout_pad / 8) / 256 >= ((int64_t)1 << 31))
        return fail(MAGNET_E_DIM, "%s: rows=%lld too large for the reduce launch", who, (long long)b.rows);
    *bytes = (int64_t)split_k * b.rows * b.cout_pad * 4;
    return 0;
}

static int64_t conv_splitk_bytes(const MagnetConvExArgs* a, bool f16d, int32_t split_k) {
    int64_t bytes = 0;
    const int rc = conv_splitk_check(a, split_k, &bytes, f16d);
    return rc ? -(int64_t)rc : bytes;
}

// A split-K call: the form, the workspace pointer, the activation, then the launch
static int conv_splitk_run(const MagnetConvExArgs* a, bool f16d, int32_t split_k, float* work, int64_t work_bytes, void* stream) {
    const char* who = conv_splitk_who(f16d);
    int64_t bytes = 0;
    if (const int rc = conv_splitk_check(a, split_k, &bytes, f16d)) return rc;
    if (!work) return fail(MAGNET_E_NULL, "%s: work is NULL", who);
    if (!aligned16(work)) return fail(MAGNET_E_ALIGN, "%s: work must be 16-byte aligned", who);
    if (work_bytes < bytes) return fail(MAGNET_E_DIM, "%s: work_bytes=%lld < %lld", who, (long long)work_bytes, (long long)bytes);
    if (const int rc = conv_act_check(a, who, false)) return rc;
    return conv_mfma_run(a, f16d ? CONV_F16D : CONV_BF16X3, split_k, work, stream);
}

MAGNET_API int64_t magnet_conv_mfma_splitk_workspace(const MagnetConvExArgs* a, int32_t split_k) { return conv_splitk_bytes(a, false, split_k); }
MAGNET_API int magnet_conv_mfma_splitk(const MagnetConvExArgs* a, int32_t split_k, float* work, int64_t work_bytes, void* stream) {
    return conv_splitk_run(a, false, split_k, work, work_bytes, stream);
}

MAGNET_API int magnet_conv_mfma_f16d(const MagnetConvExArgs* a, void* stream) {
    if (const int rc = conv_f16d_check(a, "magnet_conv_mfma_f16d")) return rc;
    return conv_mfma_run(a, CONV_F16D, 0, nullptr, stream);
}
MAGNET_API int64_t magnet_conv_mfma_f16d_splitk_workspace(const MagnetConvExArgs* a, int32_t split_k) { return conv_splitk_bytes(a, true, split_k); }
MAGNET_API int magnet_conv_mfma_f16d_splitk(const MagnetConvExArgs* a, int32_t split_k, float* work, int64_t work_bytes, void* stream) {
    return conv_splitk_run(a, true, split_k, work, work_bytes, stream);
}

// What magnet_pack_split and magnet_pack_f16 check alike, in their common order: NULL pointers, the dimensions with the c_off / ctot
// granule (8 channels, the 16-byte vector), then 16-byte alignment.  `out` holds the entry point's n_out outputs.  Where they differ,
// and stay different because each refusal is part of its entry point's contract:
//   split  takes any in_img_stride and any row count;
//   f16    refuses in_img_stride < 0 and N (h+2) (w+2) >= 2^31 as bad dims.
// The alignment messages name "outputs" and "output" accordingly.  *stride receives the image stride in floats.
static int pack_check(bool f16, const char* who, const float* nchw, void* const* out, int n_out, int32_t N, int32_t C, int32_t h,
                      int32_t w, int32_t ctot, int32_t c_off, int64_t in_img_stride, long long* stride) {
    const int g = 8;
    bool null = !nchw;
    for (int i = 0; i < n_out; ++i) null = null || !out[i];
    if (null) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (N <= 0 || C <= 0 || h <= 0 || w <= 0 || (ctot % g) != 0 || (c_off % g) != 0 || c_off < 0 || c_off + ((C + g - 1) / g) * g > ctot ||
        (f16 && (in_img_stride < 0 || (int64_t)N * (h + 2) * (w + 2) >= ((int64_t)1 << 31))))
        return fail(MAGNET_E_DIM, "%s: bad dims N=%d C=%d h=%d w=%d ctot=%d c_off=%d", who, N, C, h, w, ctot, c_off);
    *stride = in_img_stride ? (long long)in_img_stride : (long long)C * h * w;
    bool misaligned = false;
    for (int i = 0; i < n_out; ++i) misaligned = misaligned || !aligned16(out[i]);
    if (misaligned) return fail(MAGNET_E_ALIGN, "%s: %s not 16-byte aligned", who, n_out == 2 ? "outputs" : "output");
    return 0;
}

MAGNET_API int magnet_pack_f16(const float* nchw, void* out_f16, int32_t N, int32_t C, int32_t h, int32_t w, int32_t ctot, int32_t c_off,
                               int64_t in_img_stride, void* stream) {
    long long stride;
    if (const int rc = pack_check(true, "magnet_pack_f16", nchw, &out_f16, 1, N, C, h, w, ctot, c_off, in_img_stride, &stride)) return rc;
    hipError_t e = magnet::launch_pack_f16(nchw, (uint16_t*)out_f16, N, C, h, w, ctot, c_off, stride, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_pack_f16 launch");
}

MAGNET_API int magnet_planes_to_f16(const void* in_hi, const void* in_lo, int32_t ld, void* out_f16, int32_t ld16, int64_t rows, int32_t c0,
                                    int32_t c1, void* stream) {
    if (!in_hi || !in_lo || !out_f16) return fail(MAGNET_E_NULL, "magnet_planes_to_f16: NULL pointer");
    if (rows <= 0 || rows >= ((int64_t)1 << 31) || c0 < 0 || c1 <= c0 || (c0 % 8) != 0 || (c1 % 8) != 0 || (ld % 8) != 0 || (ld16 % 8) != 0 || c1 > ld || c1 > ld16)
        return fail(MAGNET_E_DIM, "magnet_planes_to_f16: bad dims rows=%lld ld=%d ld16=%d c0=%d c1=%d (multiples of 8, c0 < c1 <= ld, ld16)", (long long)rows, ld, ld16, c0, c1);
    if (!aligned16(in_hi) || !aligned16(in_lo) || !aligned16(out_f16)) return fail(MAGNET_E_ALIGN, "magnet_planes_to_f16: pointers not 16-byte aligned");
    hipError_t e = magnet::launch_planes_to_f16((const uint16_t*)in_hi, (const uint16_t*)in_lo, (uint16_t*)out_f16, rows, ld, ld16, c0, c1, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_planes_to_f16 launch");
}

MAGNET_API int64_t magnet_conv_row_tiles(int32_t n_img, int32_t h, int32_t wp, int32_t bm, int32_t* tiles_per_img) {
    int per = 0;
    if (n_img <= 0 || h <= 0 || wp < 3 || bm <= 0) { if (tiles_per_img) *tiles_per_img = 0; return 0; }
    const long long n = magnet::conv_row_tiles(n_img, h, wp, bm, &per);
    if (tiles_per_img) *tiles_per_img = per;
    return n;
}

MAGNET_API int magnet_dnet_gauss_head(const float* in, int32_t in_ld, int32_t N, int32_t h, int32_t w, int32_t pad, float* out,
                                      void* stream) {
    if (!in || !out) return fail(MAGNET_E_NULL, "magnet_dnet_gauss_head: NULL pointer");
    if (N <= 0 || h <= 0 || w <= 0 || pad < 0 || in_ld < 2 || (in_ld % 2) != 0)
        return fail(MAGNET_E_DIM, "magnet_dnet_gauss_head: bad dims N=%d h=%d w=%d pad=%d in_ld=%d (in_ld even, >= 2)", N, h, w, pad, in_ld);
    if ((reinterpret_cast<uintptr_t>(in) & 7u) || (reinterpret_cast<uintptr_t>(out) & 3u))
        return fail(MAGNET_E_ALIGN, "magnet_dnet_gauss_head: `in` must be 8-byte aligned");
    hipError_t e = magnet::launch_dnet_gauss_head(in, in_ld, N, h, w, pad, out, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_dnet_gauss_head launch");
}

MAGNET_API int magnet_dnet_upsample_gauss(const float* head, int32_t head_ld, const float* mask, int32_t mask_ld, int32_t N, int32_t h,
                                          int32_t w, float* out, void* stream) {
    if (!head || !mask || !out) return fail(MAGNET_E_NULL, "magnet_dnet_upsample_gauss: NULL pointer");
    if (N <= 0 || h <= 0 || w <= 0 || head_ld < 2 || (head_ld & 1) || mask_ld < 144 || (mask_ld % 4) ||
        (long long)N * h * w * 4 > 0x7fffffffLL * 256)
        return fail(MAGNET_E_DIM, "magnet_dnet_upsample_gauss: bad dims N=%d h=%d w=%d head_ld=%d mask_ld=%d (head_ld even, >= 2; mask_ld >= 144, "
                                  "mask_ld %% 4 == 0)", N, h, w, head_ld, mask_ld);
    if ((reinterpret_cast<uintptr_t>(head) & 7) || !aligned16(mask) || !aligned16(out))
        return fail(MAGNET_E_ALIGN, "magnet_dnet_upsample_gauss: `head` must be 8-byte, `mask` and `out` 16-byte aligned");
    hipError_t e = magnet::launch_dnet_upsample_gauss(head, head_ld, mask, mask_ld, N, h, w, out, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_dnet_upsample_gauss launch");
}

MAGNET_API int magnet_fnet_stem(const float* img, const float* wgt, const float* bias, void* out_hi, void* out_lo, int32_t N,
                                int32_t H, int32_t W, void* stream) {
    if (!img || !wgt || !bias || !out_hi || !out_lo) return fail(MAGNET_E_NULL, "magnet_fnet_stem: NULL pointer");
    if (N <= 0 || H < 2 || W < 2) return fail(MAGNET_E_DIM, "magnet_fnet_stem: bad dims N=%d H=%d W=%d", N, H, W);
    if (!aligned16(out_hi) || !aligned16(out_lo)) return fail(MAGNET_E_ALIGN, "magnet_fnet_stem: outputs must be 16-byte aligned");
    hipError_t e = magnet::launch_fnet_stem(img, wgt, bias, (uint16_t*)out_hi, (uint16_t*)out_lo, N, H, W, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_stem launch");
}

MAGNET_API int magnet_space_to_depth(const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int32_t N, int32_t C,
                                     int32_t H2, int32_t W2, int32_t opad, void* stream) {
    if (!in_hi || !in_lo || !out_hi || !out_lo) return fail(MAGNET_E_NULL, "magnet_space_to_depth: NULL pointer");
    if (N <= 0 || C <= 0 || (C % 8) != 0 || H2 <= 0 || W2 <= 0 || opad < 0)
        return fail(MAGNET_E_DIM, "magnet_space_to_depth: bad dims N=%d C=%d H2=%d W2=%d opad=%d", N, C, H2, W2, opad);
    if (!aligned16(in_hi) || !aligned16(in_lo) || !aligned16(out_hi) || !aligned16(out_lo))
        return fail(MAGNET_E_ALIGN, "magnet_space_to_depth: pointers must be 16-byte aligned");
    hipError_t e = magnet::launch_space_to_depth((const uint16_t*)in_hi, (const uint16_t*)in_lo, (uint16_t*)out_hi, (uint16_t*)out_lo,
                                                 N, C, H2, W2, opad, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_space_to_depth launch");
}

MAGNET_API int magnet_avgpool_cl(const void* in_hi, const void* in_lo, int32_t ld, int32_t N, int32_t h, int32_t w, int32_t pad,
                                 int32_t k, int32_t C, void* out_hi, void* out_lo, void* stream) {
    if (!in_hi || !in_lo || !out_hi || !out_lo) return fail(MAGNET_E_NULL, "magnet_avgpool_cl: NULL pointer");
    if (N <= 0 || C <= 0 || C > 128 || (C % 8) != 0 || ld < C || (ld % 8) != 0 || k <= 0 || h < k || w < k || pad < 0)
        return fail(MAGNET_E_DIM, "magnet_avgpool_cl: bad dims N=%d C=%d ld=%d h=%d w=%d k=%d pad=%d", N, C, ld, h, w, k, pad);
    if (!aligned16(in_hi) || !aligned16(in_lo) || !aligned16(out_hi) || !aligned16(out_lo))
        return fail(MAGNET_E_ALIGN, "magnet_avgpool_cl: pointers must be 16-byte aligned");
    hipError_t e = magnet::launch_avgpool_cl((const uint16_t*)in_hi, (const uint16_t*)in_lo, ld, N, h, w, pad, k, C, (uint16_t*)out_hi,
                                             (uint16_t*)out_lo, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_avgpool_cl launch");
}

MAGNET_API int magnet_upsample_bilinear_cl(const float* in, int32_t in_ld, int32_t ph, int32_t pw, int32_t C, void* out_hi,
                                           void* out_lo, int32_t out_ld, int32_t N, int32_t h, int32_t w, int32_t pad, void* stream) {
    if (!in || !out_hi || !out_lo) return fail(MAGNET_E_NULL, "magnet_upsample_bilinear_cl: NULL pointer");
    if (N <= 0 || C <= 0 || (C % 8) != 0 || in_ld < C || out_ld < C || (out_ld % 8) != 0 || ph <= 0 || pw <= 0 || h <= 0 || w <= 0 || pad < 0)
        return fail(MAGNET_E_DIM, "magnet_upsample_bilinear_cl: bad dims");
    if (!aligned16(out_hi) || !aligned16(out_lo)) return fail(MAGNET_E_ALIGN, "magnet_upsample_bilinear_cl: outputs must be 16-byte aligned");
    hipError_t e = magnet::launch_upsample_bilinear_cl(in, in_ld, ph, pw, C, (uint16_t*)out_hi, (uint16_t*)out_lo, out_ld, N, h, w, pad,
                                                       (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_upsample_bilinear_cl launch");
}

MAGNET_API int magnet_fnet_stem_f16(const float* img, const float* wgt, const float* bias, void* out_f16, int32_t N, int32_t H, int32_t W,
                                    void* stream) {
    if (!img || !wgt || !bias || !out_f16) return fail(MAGNET_E_NULL, "magnet_fnet_stem_f16: NULL pointer");
    if (N <= 0 || H < 2 || W < 2) return fail(MAGNET_E_DIM, "magnet_fnet_stem_f16: bad dims N=%d H=%d W=%d", N, H, W);
    if (!aligned16(out_f16)) return fail(MAGNET_E_ALIGN, "magnet_fnet_stem_f16: output must be 16-byte aligned");
    hipError_t e = magnet::launch_fnet_stem_f16(img, wgt, bias, (uint16_t*)out_f16, N, H, W, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_stem_f16 launch");
}

MAGNET_API int magnet_space_to_depth_f16(const void* in_f16, void* out_f16, int32_t N, int32_t C, int32_t H2, int32_t W2, int32_t opad,
                                         void* stream) {
    if (!in_f16 || !out_f16) return fail(MAGNET_E_NULL, "magnet_space_to_depth_f16: NULL pointer");
    if (N <= 0 || C <= 0 || (C % 8) != 0 || H2 <= 0 || W2 <= 0 || opad < 0)
        return fail(MAGNET_E_DIM, "magnet_space_to_depth_f16: bad dims N=%d C=%d H2=%d W2=%d opad=%d", N, C, H2, W2, opad);
    if (!aligned16(in_f16) || !aligned16(out_f16)) return fail(MAGNET_E_ALIGN, "magnet_space_to_depth_f16: pointers must be 16-byte aligned");
    hipError_t e = magnet::launch_space_to_depth_f16((const uint16_t*)in_f16, (uint16_t*)out_f16, N, C, H2, W2, opad, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_space_to_depth_f16 launch");
}

MAGNET_API int magnet_avgpool_cl_f16(const void* in_f16, int32_t ld, int32_t N, int32_t h, int32_t w, int32_t pad, int32_t k, int32_t C,
                                     void* out_f16, void* stream) {
    if (!in_f16 || !out_f16) return fail(MAGNET_E_NULL, "magnet_avgpool_cl_f16: NULL pointer");
    if (N <= 0 || C <= 0 || C > 128 || (C % 8) != 0 || ld < C || (ld % 8) != 0 || k <= 0 || h < k || w < k || pad < 0)
        return fail(MAGNET_E_DIM, "magnet_avgpool_cl_f16: bad dims N=%d C=%d ld=%d h=%d w=%d k=%d pad=%d", N, C, ld, h, w, k, pad);
    if (!aligned16(in_f16) || !aligned16(out_f16)) return fail(MAGNET_E_ALIGN, "magnet_avgpool_cl_f16: pointers must be 16-byte aligned");
    hipError_t e = magnet::launch_avgpool_cl_f16((const uint16_t*)in_f16, ld, N, h, w, pad, k, C, (uint16_t*)out_f16, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_avgpool_cl_f16 launch");
}

MAGNET_API int magnet_upsample_bilinear_cl_f16(const float* in, int32_t in_ld, int32_t ph, int32_t pw, int32_t C, void* out_f16,
                                               int32_t out_ld, int32_t N, int32_t h, int32_t w, int32_t pad, void* stream) {
    if (!in || !out_f16) return fail(MAGNET_E_NULL, "magnet_upsample_bilinear_cl_f16: NULL pointer");
    if (N <= 0 || C <= 0 || (C % 8) != 0 || in_ld < C || out_ld < C || (out_ld % 8) != 0 || ph <= 0 || pw <= 0 || h <= 0 || w <= 0 || pad < 0)
        return fail(MAGNET_E_DIM, "magnet_upsample_bilinear_cl_f16: bad dims");
    if (!aligned16(out_f16)) return fail(MAGNET_E_ALIGN, "magnet_upsample_bilinear_cl_f16: output must be 16-byte aligned");
    hipError_t e = magnet::launch_upsample_bilinear_cl_f16(in, in_ld, ph, pw, C, (uint16_t*)out_f16, out_ld, N, h, w, pad, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_upsample_bilinear_cl_f16 launch");
}

MAGNET_API int magnet_pack_split(const float* nchw, void* out_hi, void* out_lo, int32_t N, int32_t C, int32_t h, int32_t w,
                                 int32_t ctot, int32_t c_off, int64_t in_img_stride, void* stream) {
    void* const out[2] = {out_hi, out_lo};
    long long stride;
    if (const int rc = pack_check(false, "magnet_pack_split", nchw, out, 2, N, C, h, w, ctot, c_off, in_img_stride, &stride)) return rc;
    hipError_t e = magnet::launch_pack_split(nchw, (uint16_t*)out_hi, (uint16_t*)out_lo, N, C, h, w, ctot, c_off, stride, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_pack_split launch");
}

MAGNET_API int magnet_gaussian_update_cl(const float* gnet_out_pad, int32_t ld, const float* gmm_in, float* gmm_out,
                                         int32_t B, int32_t h, int32_t w, void* stream) {
    if (!gnet_out_pad || !gmm_in || !gmm_out) return fail(MAGNET_E_NULL, "magnet_gaussian_update_cl: NULL pointer");
    if (B <= 0 || h <= 0 || w <= 0 || ld < 2) return fail(MAGNET_E_DIM, "magnet_gaussian_update_cl: bad dims");
    hipError_t e = magnet::launch_gaussian_update_cl(gnet_out_pad, ld, gmm_in, gmm_out, B, h, w, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_gaussian_update_cl launch");
}

MAGNET_API int magnet_upsample_depth_cl(const float* depth, const float* mask_pad, int32_t ld, float* out, int32_t B,
                                        int32_t h, int32_t w, void* stream) {
    if (!depth || !mask_pad || !out) return fail(MAGNET_E_NULL, "magnet_upsample_depth_cl: NULL pointer");
    if (B <= 0 || h <= 0 || w <= 0 || ld < 144 || (ld % 4)) return fail(MAGNET_E_DIM, "magnet_upsample_depth_cl: bad dims (ld >= 144, ld %% 4 == 0)");
    if (!aligned16(out) || !aligned16(mask_pad)) return fail(MAGNET_E_ALIGN, "magnet_upsample_depth_cl: pointers not 16-byte aligned");
    hipError_t e = magnet::launch_upsample_cl(depth, mask_pad, ld, out, B, h, w, 1, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_upsample_depth_cl launch");
}

MAGNET_API int magnet_upsample_depth_cl_n(const float* depths, const float* mask_pad, int32_t ld, float* outs, int32_t n_pred, int32_t B,
                                          int32_t h, int32_t w, void* stream) {
    if (!depths || !mask_pad || !outs) return fail(MAGNET_E_NULL, "magnet_upsample_depth_cl_n: NULL pointer");
    if (n_pred <= 0 || n_pred > 64 || B <= 0 || h <= 0 || w <= 0 || ld < 144 || (ld % 4))
        return fail(MAGNET_E_DIM, "magnet_upsample_depth_cl_n: bad dims (1 <= n_pred <= 64, ld >= 144, ld %% 4 == 0)");
    if (!aligned16(outs) || !aligned16(mask_pad)) return fail(MAGNET_E_ALIGN, "magnet_upsample_depth_cl_n: pointers not 16-byte aligned");
    hipError_t e = magnet::launch_upsample_cl(depths, mask_pad, ld, outs, B, h, w, n_pred, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_upsample_depth_cl_n launch");
}

MAGNET_API int magnet_depth_metrics(const float* pred, const float* gt, double* sums, int32_t B, int32_t HW, float min_depth,
                                    float max_depth, void* stream) {
    if (!pred || !gt || !sums) return fail(MAGNET_E_NULL, "magnet_depth_metrics: NULL pointer");
    if (B <= 0 || HW <= 0 || !(max_depth > min_depth)) return fail(MAGNET_E_DIM, "magnet_depth_metrics: bad arguments");
    hipError_t e = magnet::launch_depth_metrics(pred, gt, sums, B, HW, HW, min_depth, max_depth, 0, -1, 0, 0, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_depth_metrics launch");
}

MAGNET_API int magnet_depth_metrics_crop(const float* pred, const float* gt, double* sums, int32_t B, int32_t H, int32_t W,
                                         float min_depth, float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1, void* stream) {
    if (!pred || !gt || !sums) return fail(MAGNET_E_NULL, "magnet_depth_metrics_crop: NULL pointer");
    if (B <= 0 || H <= 0 || W <= 0 || !(max_depth > min_depth) || y0 < 0 || x0 < 0 || y1 > H || x1 > W || y1 < y0 || x1 < x0)
        return fail(MAGNET_E_DIM, "magnet_depth_metrics_crop: bad arguments");
    hipError_t e = magnet::launch_depth_metrics(pred, gt, sums, B, H * W, W, min_depth, max_depth, y0, y1, x0, x1, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_depth_metrics_crop launch");
}

MAGNET_API int64_t magnet_depth_metrics_workspace(int32_t B) {
    if (B <= 0) return -(int64_t)fail(MAGNET_E_DIM, "magnet_depth_metrics_workspace: bad B=%d", B);
    return magnet::depth_metrics_workspace_bytes(B);
}

static bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

MAGNET_API int magnet_depth_metrics_ex(const MagnetDepthMetricsArgs* a, void* stream) {
    if (!a || !a->mu || !a->gt || !a->work || (!a->sums && !a->rows)) return fail(MAGNET_E_NULL, "magnet_depth_metrics_ex: NULL pointer");
    if (a->B <= 0 || a->H <= 0 || a->W <= 0 || (long long)a->H * a->W > 0x7fffffffLL - 64 * 256 || !(a->max_depth > a->min_depth))
        return fail(MAGNET_E_DIM, "magnet_depth_metrics_ex: bad arguments B=%d H=%d W=%d", a->B, a->H, a->W);
    if (a->kind != MAGNET_METRICS_SIGMA && a->kind != MAGNET_METRICS_VARIANCE && a->kind != MAGNET_METRICS_NONE)
        return fail(MAGNET_E_DIM, "magnet_depth_metrics_ex: unknown kind %d", a->kind);
    if ((a->kind == MAGNET_METRICS_NONE) != (a->second == nullptr))
        return fail(MAGNET_E_DIM, "magnet_depth_metrics_ex: second must be NULL exactly when kind is MAGNET_METRICS_NONE");
    if (a->crop && (a->y0 < 0 || a->x0 < 0 || a->y1 > a->H || a->x1 > a->W || a->y1 <= a->y0 || a->x1 <= a->x0))
        return fail(MAGNET_E_DIM, "magnet_depth_metrics_ex: empty or out-of-frame crop [%d,%d) x [%d,%d)", a->y0, a->y1, a->x0, a->x1);
    if (!aligned8(a->sums) || !aligned8(a->rows) || !aligned8(a->work))
        return fail(MAGNET_E_ALIGN, "magnet_depth_metrics_ex: sums / rows / work not 8-byte aligned");
    hipError_t e = magnet::launch_depth_metrics_ex(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_depth_metrics_ex launch");
}

// ---- training step (train_bwd.hip) ----
MAGNET_API int magnet_nll_loss_forward(const MagnetNllArgs* a, void* stream) {
    if (!a || !a->preds || !a->gt || !a->mask || !a->sums || !a->loss || !a->work)
        return fail(MAGNET_E_NULL, "magnet_nll_loss_forward: NULL pointer");
    if (a->n_iter <= 0 || a->n_iter > MAGNET_NLL_MAX_ITER || a->B <= 0 || a->H <= 0 || a->W <= 0)
        return fail(MAGNET_E_DIM, "magnet_nll_loss_forward: bad dims (1 <= n_iter <= %d)", MAGNET_NLL_MAX_ITER);
    hipError_t e = magnet::launch_nll_forward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_nll_loss_forward launch");
}

MAGNET_API int magnet_nll_loss_backward(const MagnetNllArgs* a, void* stream) {
    if (!a || !a->preds || !a->gt || !a->mask || !a->sums || !a->grad_loss || !a->grad_preds)
        return fail(MAGNET_E_NULL, "magnet_nll_loss_backward: NULL pointer");
    if (a->n_iter <= 0 || a->n_iter > MAGNET_NLL_MAX_ITER || a->B <= 0 || a->H <= 0 || a->W <= 0)
        return fail(MAGNET_E_DIM, "magnet_nll_loss_backward: bad dims (1 <= n_iter <= %d)", MAGNET_NLL_MAX_ITER);
    hipError_t e = magnet::launch_nll_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_nll_loss_backward launch");
}

MAGNET_API int magnet_upsample_depth_backward(const MagnetUpsampleBwdArgs* a, void* stream) {
    if (!a || !a->grad_up || !a->depth || !a->mask || !a->grad_depth || !a->grad_mask || !a->work)
        return fail(MAGNET_E_NULL, "magnet_upsample_depth_backward: NULL pointer");
    if (a->n_pred <= 0 || a->B <= 0 || a->h <= 0 || a->w <= 0 || a->k <= 0 || a->k > 8)
        return fail(MAGNET_E_DIM, "magnet_upsample_depth_backward: bad dims (1 <= k <= 8)");
    hipError_t e = magnet::launch_upsample_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_upsample_depth_backward launch");
}

MAGNET_API int magnet_head_dgrad(const MagnetHeadDgradArgs* a, void* stream) {
    if (!a || !a->wt_hi || !a->wt_lo || !a->h3_hi || !a->h2_hi || !a->h1_hi || !a->dout_hi || !a->dout_lo || !a->dh3_hi ||
        !a->dh3_lo || !a->dh2_hi || !a->dh2_lo || !a->dh1_hi || !a->dh1_lo)
        return fail(MAGNET_E_NULL, "magnet_head_dgrad: NULL pointer");
    if (!a->dout && (!a->grad_gmm || !a->gnet_out || !a->gmm_in)) return fail(MAGNET_E_NULL, "magnet_head_dgrad: NULL pointer (G-Net form)");
    if (a->acc_mode && !a->acc) return fail(MAGNET_E_NULL, "magnet_head_dgrad: acc_mode without acc");
    if ((a->acc_hi == nullptr) != (a->acc_lo == nullptr)) return fail(MAGNET_E_NULL, "magnet_head_dgrad: acc_hi / acc_lo");
    if (a->B <= 0 || a->h <= 0 || a->w <= 0 || a->rows != (int64_t)a->B * (a->h + 2) * (a->w + 2) ||
        (a->k0 != 32 && a->k0 != 128 && a->k0 != 160) || (!a->dout && (a->k0 != 32 || a->gnet_ld < 2)) ||
        a->acc_mode < 0 || a->acc_mode > 2 || (a->acc && !a->acc_mode))
        return fail(MAGNET_E_DIM, "magnet_head_dgrad: bad dims (rows = B(h+2)(w+2), k0 in {32,128,160}, G-Net form k0 = 32)");
    const void* al[] = {a->dout, a->wt_hi, a->wt_lo, a->h3_hi, a->h2_hi, a->h1_hi, a->dout_hi, a->dout_lo, a->dh3_hi, a->dh3_lo,
                        a->dh2_hi, a->dh2_lo, a->dh1_hi, a->dh1_lo, a->acc, a->acc_hi, a->acc_lo};
    for (const void* p : al) if (!aligned16(p)) return fail(MAGNET_E_ALIGN, "magnet_head_dgrad: pointers not 16-byte aligned");
    hipError_t e = magnet::launch_head_dgrad(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_head_dgrad launch");
}

static int wgrad_check(const MagnetWgradArgs* a, const char* who) {
    if (!a || !a->dy_hi || !a->dy_lo || !a->x_hi || !a->x_lo || !a->grad_w) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (a->cout <= 0 || a->cin <= 0 || (a->cout % 8) || (a->cin % 8) || (a->taps != 1 && a->taps != 9) || a->wp < 1 ||
        a->rows <= 0 || a->dy_ld < a->cout || a->x_ld < a->cin || (a->dy_ld % 8) || (a->x_ld % 8) ||
        a->cout_valid <= 0 || a->cout_valid > a->cout || a->cin_valid <= 0 || a->cin_valid > a->cin || a->cin_dst < 0 ||
        a->cin_dst + a->cin_valid > a->cin_total)
        return fail(MAGNET_E_DIM, "%s: bad dims (cout, cin, ld multiples of 8; taps 1 or 9; valid ranges inside)", who);
    return 0;
}

MAGNET_API int64_t magnet_wgrad_workspace(const MagnetWgradArgs* a) {
    if (int rc = wgrad_check(a, "magnet_wgrad_workspace")) return -(int64_t)rc;
    return magnet::wgrad_workspace_bytes(*a);
}

MAGNET_API int magnet_wgrad(const MagnetWgradArgs* a, void* stream) {
    if (int rc = wgrad_check(a, "magnet_wgrad")) return rc;
    if (!a->work && magnet::wgrad_workspace_bytes(*a) > 0) return fail(MAGNET_E_NULL, "magnet_wgrad: NULL workspace");
    const void* al[] = {a->dy_hi, a->dy_lo, a->x_hi, a->x_lo, a->work};
    for (const void* p : al) if (!aligned16(p)) return fail(MAGNET_E_ALIGN, "magnet_wgrad: pointers not 16-byte aligned");
    hipError_t e = magnet::launch_wgrad(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_wgrad launch");
}

// ---- F-Net forward in training mode (train_fnet_fwd.hip) ----
MAGNET_API int magnet_fnet_stem_raw(const float* img, const float* wgt, float* out, int32_t N, int32_t H, int32_t W, void* stream) {
    if (!img || !wgt || !out) return fail(MAGNET_E_NULL, "magnet_fnet_stem_raw: NULL pointer");
    if (N <= 0 || H < 2 || W < 2) return fail(MAGNET_E_DIM, "magnet_fnet_stem_raw: bad dims N=%d H=%d W=%d", N, H, W);
    if (!aligned16(out)) return fail(MAGNET_E_ALIGN, "magnet_fnet_stem_raw: output must be 16-byte aligned");
    hipError_t e = magnet::launch_fnet_stem_raw(img, wgt, out, N, H, W, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_stem_raw launch");
}

// min_pos: 2 where the launch takes the variance of these positions alone, 1 where the statistics come from elsewhere
static int bn_train_check(const MagnetBnTrainArgs* a, const char* who, int min_pos = 2, bool stats_out = true) {
    if (!a || !a->x || (stats_out && (!a->mean || !a->invstd))) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (a->N <= 0 || a->C <= 0 || a->C > 2048 || (a->C % 8) || a->pad < 0 || a->hp <= 2 * a->pad || a->wp <= 2 * a->pad || a->x_ld < a->C ||
        (a->x_ld % 4) || (long long)a->N * (a->hp - 2 * a->pad) * (a->wp - 2 * a->pad) < min_pos)
        return fail(MAGNET_E_DIM, "%s: bad dims (C a multiple of 8 up to 2048, x_ld >= C a multiple of 4, at least %d position(s))", who,
                    min_pos);
    if (!aligned16(a->x)) return fail(MAGNET_E_ALIGN, "%s: x must be 16-byte aligned", who);
    return 0;
}

MAGNET_API int magnet_bn_train_stats(const MagnetBnTrainArgs* a, void* stream) {
    if (int rc = bn_train_check(a, "magnet_bn_train_stats")) return rc;
    if (!a->work) return fail(MAGNET_E_NULL, "magnet_bn_train_stats: NULL workspace");
    if (!(a->eps >= 0.0) || a->momentum > 1.0) return fail(MAGNET_E_DIM, "magnet_bn_train_stats: eps >= 0 and momentum <= 1 required");
    hipError_t e = magnet::launch_bn_train_stats(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_bn_train_stats launch");
}

MAGNET_API int magnet_bn_train_apply(const MagnetBnTrainArgs* a, void* stream) {
    if (int rc = bn_train_check(a, "magnet_bn_train_apply", 1)) return rc;
    if (!a->gamma || !a->beta || (!a->out_f32 && (!a->out_hi || !a->out_lo))) return fail(MAGNET_E_NULL, "magnet_bn_train_apply: NULL pointer");
    if ((a->res_hi == nullptr) != (a->res_lo == nullptr)) return fail(MAGNET_E_NULL, "magnet_bn_train_apply: res_hi and res_lo come together");
    if (a->out_ld < a->C || (a->out_f32 ? (a->out_ld % 4) : (a->out_ld % 8)) || (a->res_hi && (a->res_ld < a->C || (a->res_ld % 8))))
        return fail(MAGNET_E_DIM, "magnet_bn_train_apply: out_ld / res_ld must be >= C and multiples of 8 (4 for fp32 output)");
    const void* al[] = {a->out_f32, a->out_hi, a->out_lo, a->res_hi, a->res_lo};
    for (const void* p : al) if (!aligned16(p)) return fail(MAGNET_E_ALIGN, "magnet_bn_train_apply: pointers not 16-byte aligned");
    hipError_t e = magnet::launch_bn_train_apply(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_bn_train_apply launch");
}

// ---- F-Net backward in training mode (train_fnet_bwd.hip, train_bwd.hip) ----
static int wgrad_ex_check(const MagnetWgradExArgs* e, const char* who) {
    if (!e) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    const MagnetWgradArgs* a = &e->base;
    if (!a->dy_hi || !a->dy_lo || !a->x_hi || !a->x_lo || !a->grad_w) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (a->cout <= 0 || a->cin <= 0 || (a->cout % 8) || (a->cin % 8) || (a->taps != 1 && a->taps != 4 && a->taps != 9) || a->wp < 3 ||
        e->dil < 0 || e->dil > 8 || a->rows <= 0 || a->dy_ld < a->cout || a->x_ld < a->cin || (a->dy_ld % 8) || (a->x_ld % 8) ||
        a->cout_valid <= 0 || a->cout_valid > a->cout || a->cin_valid <= 0 || a->cin_valid > a->cin || a->cin_dst < 0 ||
        a->cin_dst + a->cin_valid > a->cin_total)
        return fail(MAGNET_E_DIM, "%s: bad dims (cout, cin, ld multiples of 8; taps 1, 4 or 9; dil <= 8; valid ranges inside)", who);
    return 0;
}

MAGNET_API int64_t magnet_wgrad_ex_workspace(const MagnetWgradExArgs* e) {
    if (int rc = wgrad_ex_check(e, "magnet_wgrad_ex_workspace")) return -(int64_t)rc;
    return magnet::wgrad_ex_workspace_bytes(*e);
}

MAGNET_API int magnet_wgrad_ex(const MagnetWgradExArgs* e, void* stream) {
    if (int rc = wgrad_ex_check(e, "magnet_wgrad_ex")) return rc;
    const MagnetWgradArgs* a = &e->base;
    if (!a->work && magnet::wgrad_ex_workspace_bytes(*e) > 0) return fail(MAGNET_E_NULL, "magnet_wgrad_ex: NULL workspace");
    const void* al[] = {a->dy_hi, a->dy_lo, a->x_hi, a->x_lo, a->work};
    for (const void* p : al) if (!aligned16(p)) return fail(MAGNET_E_ALIGN, "magnet_wgrad_ex: pointers not 16-byte aligned");
    hipError_t err = magnet::launch_wgrad_ex(*e, (hipStream_t)stream);
    return err == hipSuccess ? 0 : hip_fail(err, "magnet_wgrad_ex launch");
}

MAGNET_API int magnet_bn_train_backward(const MagnetBnBwdArgs* a, void* stream) {
    if (!a || !a->x || !a->mean || !a->invstd || !a->gamma || !a->beta || !a->g || !a->work || !a->dgamma || !a->dbeta || !a->dx_hi ||
        !a->dx_lo)
        return fail(MAGNET_E_NULL, "magnet_bn_train_backward: NULL pointer");
    if (a->N <= 0 || a->C <= 0 || a->pad < 0 || a->hp <= 2 * a->pad || a->wp <= 2 * a->pad || a->x_ld < a->C || a->g_ld < a->C ||
        a->dx_ld < a->C || (long long)a->N * (a->hp - 2 * a->pad) * (a->wp - 2 * a->pad) < 2)
        return fail(MAGNET_E_DIM, "magnet_bn_train_backward: bad dims");
    hipError_t e = magnet::launch_bn_train_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_bn_train_backward launch");
}

MAGNET_API int magnet_fnet_grad_pack(const float* nchw, void* out_hi, void* out_lo, int32_t N, int32_t C, int32_t h, int32_t w,
                                     int32_t pad, int32_t ld, void* stream) {
    if (!nchw || !out_hi || !out_lo) return fail(MAGNET_E_NULL, "magnet_fnet_grad_pack: NULL pointer");
    if (N <= 0 || C <= 0 || h <= 0 || w <= 0 || pad < 0 || ld < C) return fail(MAGNET_E_DIM, "magnet_fnet_grad_pack: bad dims");
    hipError_t e = magnet::launch_fnet_grad_pack(nchw, (uint16_t*)out_hi, (uint16_t*)out_lo, N, C, h, w, pad, ld, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_grad_pack launch");
}

MAGNET_API int magnet_fnet_d2s_backward(const float* in, float* out, int32_t N, int32_t C, int32_t H2, int32_t W2, int32_t ipad,
                                        void* stream) {
    if (!in || !out) return fail(MAGNET_E_NULL, "magnet_fnet_d2s_backward: NULL pointer");
    if (N <= 0 || C <= 0 || H2 <= 0 || W2 <= 0 || ipad < 0) return fail(MAGNET_E_DIM, "magnet_fnet_d2s_backward: bad dims");
    hipError_t e = magnet::launch_fnet_d2s_backward(in, out, N, C, H2, W2, ipad, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_d2s_backward launch");
}

MAGNET_API int magnet_spp_upsample_backward(const MagnetSppBwdArgs* a, void* stream) {
    if (!a || !a->g || !a->dq) return fail(MAGNET_E_NULL, "magnet_spp_upsample_backward: NULL pointer");
    if (a->N <= 0 || a->h <= 0 || a->w <= 0 || a->pad < 0 || a->ph <= 0 || a->pw <= 0 || a->c_off < 0 || a->g_ld < a->c_off + 32)
        return fail(MAGNET_E_DIM, "magnet_spp_upsample_backward: bad dims");
    hipError_t e = magnet::launch_spp_upsample_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_spp_upsample_backward launch");
}

MAGNET_API int magnet_spp_pool_backward(const MagnetSppBwdArgs* a, void* stream) {
    if (!a || !a->g || !a->out || !a->dpool[0] || !a->dpool[1] || !a->dpool[2] || !a->dpool[3])
        return fail(MAGNET_E_NULL, "magnet_spp_pool_backward: NULL pointer");
    if (a->N <= 0 || a->h < 64 || a->w < 64 || a->pad < 0 || a->c_off < 0 || a->g_ld < a->c_off + 128 || a->out_ld < 128)
        return fail(MAGNET_E_DIM, "magnet_spp_pool_backward: bad dims (h, w >= 64)");
    hipError_t e = magnet::launch_spp_pool_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_spp_pool_backward launch");
}

MAGNET_API int magnet_fnet_stem_wgrad(const float* img, const void* dz_hi, const void* dz_lo, float* grad_w, double* work, int32_t N,
                                      int32_t H, int32_t W, void* stream) {
    if (!img || !dz_hi || !dz_lo || !grad_w || !work) return fail(MAGNET_E_NULL, "magnet_fnet_stem_wgrad: NULL pointer");
    if (N <= 0 || H < 2 || W < 2) return fail(MAGNET_E_DIM, "magnet_fnet_stem_wgrad: bad dims");
    hipError_t e = magnet::launch_fnet_stem_wgrad(img, (const uint16_t*)dz_hi, (const uint16_t*)dz_lo, grad_w, work, N, H, W,
                                                  (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_stem_wgrad launch");
}

static int fnet_loss_dims(const MagnetFnetLossArgs* a, const char* who) {
    if (a->D < 1 || a->D > MAGNET_MAX_CANDIDATES || a->B <= 0 || a->h <= 0 || a->w <= 0)
        return fail(MAGNET_E_DIM, "%s: bad dims B=%d D=%d h=%d w=%d (1 <= D <= %d)", who, a->B, a->D, a->h, a->w, MAGNET_MAX_CANDIDATES);
    if (!(a->min_depth >= 0.f)) return fail(MAGNET_E_DIM, "%s: min_depth must be >= 0 (the validity test assumes it)", who);
    return 0;
}

MAGNET_API int magnet_fnet_loss_forward(const MagnetFnetLossArgs* a, void* stream) {
    if (!a || !a->x || !a->d || !a->pred || (a->gt && (!a->m || !a->rz || !a->sums || !a->loss || !a->work)))
        return fail(MAGNET_E_NULL, "magnet_fnet_loss_forward: NULL pointer");
    if (int rc = fnet_loss_dims(a, "magnet_fnet_loss_forward")) return rc;
    hipError_t e = magnet::launch_fnet_loss_forward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_loss_forward launch");
}

MAGNET_API int magnet_fnet_loss_backward(const MagnetFnetLossArgs* a, void* stream) {
    if (!a || !a->x || !a->d || !a->gt || !a->pred || !a->m || !a->rz || !a->sums || !a->grad_loss || !a->grad_x)
        return fail(MAGNET_E_NULL, "magnet_fnet_loss_backward: NULL pointer");
    if (int rc = fnet_loss_dims(a, "magnet_fnet_loss_backward")) return rc;
    hipError_t e = magnet::launch_fnet_loss_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_fnet_loss_backward launch");
}

// ---- synchronised BatchNorm (train_fnet_fwd.hip, train_fnet_bwd.hip): the device arithmetic around the caller's all-gather ----
MAGNET_API int magnet_bn_sync_moments(const MagnetBnTrainArgs* a, double* record, void* stream) {
    if (!record) return fail(MAGNET_E_NULL, "magnet_bn_sync_moments: NULL record");
    if (int rc = bn_train_check(a, "magnet_bn_sync_moments", 1, false)) return rc;
    if (!a->work) return fail(MAGNET_E_NULL, "magnet_bn_sync_moments: NULL workspace");
    hipError_t e = magnet::launch_bn_sync_moments(*a, record, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_bn_sync_moments launch");
}

MAGNET_API int magnet_bn_sync_merge(const MagnetBnTrainArgs* a, const double* records, int32_t world, double* n_tot, void* stream) {
    if (!a || !records || !n_tot || !a->mean || !a->invstd) return fail(MAGNET_E_NULL, "magnet_bn_sync_merge: NULL pointer");
    if (world < 1 || a->C <= 0 || a->C > 2048 || (a->C % 8))
        return fail(MAGNET_E_DIM, "magnet_bn_sync_merge: bad dims (world >= 1, C a multiple of 8 up to 2048), world=%d C=%d", world, a->C);
    if (!(a->eps >= 0.0) || a->momentum > 1.0) return fail(MAGNET_E_DIM, "magnet_bn_sync_merge: eps >= 0 and momentum <= 1 required");
    hipError_t e = magnet::launch_bn_sync_merge(*a, records, world, n_tot, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_bn_sync_merge launch");
}

static int bn_sync_bwd_check(const MagnetBnBwdArgs* a, const char* who) {
    if (!a || !a->x || !a->mean || !a->invstd || !a->gamma || !a->beta || !a->g || !a->work) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (a->N <= 0 || a->C <= 0 || a->C > 2048 || (a->C % 8) || a->pad < 0 || a->hp <= 2 * a->pad || a->wp <= 2 * a->pad || a->x_ld < a->C ||
        a->g_ld < a->C)
        return fail(MAGNET_E_DIM, "%s: bad dims (C a multiple of 8 up to 2048, x_ld / g_ld >= C, at least 1 position)", who);
    return 0;
}

MAGNET_API int magnet_bn_sync_backward_sums(const MagnetBnBwdArgs* a, double* sums, void* stream) {
    if (!sums) return fail(MAGNET_E_NULL, "magnet_bn_sync_backward_sums: NULL sums");
    if (int rc = bn_sync_bwd_check(a, "magnet_bn_sync_backward_sums")) return rc;
    if (!a->dgamma || !a->dbeta) return fail(MAGNET_E_NULL, "magnet_bn_sync_backward_sums: NULL dgamma / dbeta");
    hipError_t e = magnet::launch_bn_sync_backward_sums(*a, sums, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_bn_sync_backward_sums launch");
}

MAGNET_API int magnet_bn_sync_backward_apply(const MagnetBnBwdArgs* a, const double* sums, int32_t world, const double* n_tot, void* stream) {
    if (!sums || !n_tot) return fail(MAGNET_E_NULL, "magnet_bn_sync_backward_apply: NULL sums / n_tot");
    if (int rc = bn_sync_bwd_check(a, "magnet_bn_sync_backward_apply")) return rc;
    if (!a->dx_hi || !a->dx_lo) return fail(MAGNET_E_NULL, "magnet_bn_sync_backward_apply: NULL dx");
    if (world < 1 || a->dx_ld < a->C) return fail(MAGNET_E_DIM, "magnet_bn_sync_backward_apply: world >= 1 and dx_ld >= C required");
    hipError_t e = magnet::launch_bn_sync_backward_apply(*a, sums, world, n_tot, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_bn_sync_backward_apply launch");
}

// ---- DnetLoss (dnet_loss.hip) ----
static int dnet_loss_dims(const MagnetDnetLossArgs* a, const char* who) {
    if (!a) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (a->k != 4) return fail(MAGNET_E_DIM, "%s: k=%d is not built (the D-Net's downsample ratio is 4)", who, a->k);
    if (a->B <= 0 || a->h <= 0 || a->w <= 0 || (long long)a->B * a->h * a->w > (1LL << 31))
        return fail(MAGNET_E_DIM, "%s: bad dims B=%d h=%d w=%d (positive, B h w <= 2^31)", who, a->B, a->h, a->w);
    return 0;
}

static int dnet_loss_common(const MagnetDnetLossArgs* a, const char* who) {
    if (!a || !a->depth || !a->mask || !a->gt || !a->valid || !a->sums || !a->work) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (int rc = dnet_loss_dims(a, who)) return rc;
    if (!aligned16(a->gt) || !aligned16(a->pred) || (reinterpret_cast<uintptr_t>(a->valid) & 3u) || (reinterpret_cast<uintptr_t>(a->work) & 7u))
        return fail(MAGNET_E_ALIGN, "%s: gt and pred must be 16-byte, work 8-byte and valid 4-byte aligned", who);
    return 0;
}

MAGNET_API int64_t magnet_dnet_loss_workspace(const MagnetDnetLossArgs* a) {
    if (int rc = dnet_loss_dims(a, "magnet_dnet_loss_workspace")) return -(int64_t)rc;
    return magnet::dnet_loss_workspace_bytes(*a);
}

MAGNET_API int magnet_dnet_loss_forward(const MagnetDnetLossArgs* a, void* stream) {
    if (int rc = dnet_loss_common(a, "magnet_dnet_loss_forward")) return rc;
    if (!a->loss) return fail(MAGNET_E_NULL, "magnet_dnet_loss_forward: NULL pointer");
    hipError_t e = magnet::launch_dnet_loss_forward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_dnet_loss_forward launch");
}

MAGNET_API int magnet_dnet_loss_backward(const MagnetDnetLossArgs* a, void* stream) {
    if (int rc = dnet_loss_common(a, "magnet_dnet_loss_backward")) return rc;
    if (!a->grad_loss || !a->grad_depth || !a->grad_mask) return fail(MAGNET_E_NULL, "magnet_dnet_loss_backward: NULL pointer");
    hipError_t e = magnet::launch_dnet_loss_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_dnet_loss_backward launch");
}

static int dnet_nll_dims(const MagnetDnetNllArgs* a, const char* who) {
    if (a->B <= 0 || a->H <= 0 || a->W <= 0) return fail(MAGNET_E_DIM, "%s: bad dims B=%d H=%d W=%d", who, a->B, a->H, a->W);
    return 0;
}

MAGNET_API int magnet_dnet_nll_forward(const MagnetDnetNllArgs* a, void* stream) {
    if (!a || !a->pred || !a->gt || !a->valid || !a->sums || !a->loss || !a->work)
        return fail(MAGNET_E_NULL, "magnet_dnet_nll_forward: NULL pointer");
    if (int rc = dnet_nll_dims(a, "magnet_dnet_nll_forward")) return rc;
    hipError_t e = magnet::launch_dnet_nll_forward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_dnet_nll_forward launch");
}

MAGNET_API int magnet_dnet_nll_backward(const MagnetDnetNllArgs* a, void* stream) {
    if (!a || !a->pred || !a->gt || !a->valid || !a->sums || !a->grad_loss || !a->grad_pred)
        return fail(MAGNET_E_NULL, "magnet_dnet_nll_backward: NULL pointer");
    if (int rc = dnet_nll_dims(a, "magnet_dnet_nll_backward")) return rc;
    hipError_t e = magnet::launch_dnet_nll_backward(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_dnet_nll_backward launch");
}

MAGNET_API int magnet_gather_views(const MagnetGatherViewsArgs* a, void* stream) {
    if (!a || !a->slots) return fail(MAGNET_E_NULL, "magnet_gather_views: NULL pointer");
    if ((a->ref_cl || a->src_pad) && !a->pool_feat) return fail(MAGNET_E_NULL, "magnet_gather_views: ref_cl / src_pad need pool_feat");
    if ((a->ref_gmm || a->src_gmm) && !a->pool_gmm) return fail(MAGNET_E_NULL, "magnet_gather_views: ref_gmm / src_gmm need pool_gmm");
    if ((a->gin_hi != nullptr) != (a->gin_lo != nullptr) || (a->gin_hi && (!a->pool_xd3_hi || !a->pool_xd3_lo)))
        return fail(MAGNET_E_NULL, "magnet_gather_views: gin_hi and gin_lo go together and need both x_d3 pool planes");
    if (a->feat_dtype != MAGNET_FEAT_F32 && a->feat_dtype != MAGNET_FEAT_BF16)
        return fail(MAGNET_E_DTYPE, "magnet_gather_views: unknown dtype %d", a->feat_dtype);
    const long long R = ((long long)a->h + 2) * ((long long)a->w + 2);
    if (a->n_slots <= 0 || a->B <= 0 || a->V < 0 || a->h <= 0 || a->w <= 0 || a->F <= 0 || (a->F % 8) != 0 ||
        (1LL + a->V) * a->B > 0x7fffffffLL || R * 32 > 0x7fffffffLL || R * a->F / 4 > 0x7fffffffLL)
        return fail(MAGNET_E_DIM, "magnet_gather_views: bad dims n_slots=%d B=%d V=%d h=%d w=%d F=%d (F must be a multiple of 8)",
                    a->n_slots, a->B, a->V, a->h, a->w, a->F);
    if (a->gin_hi && (a->gin_c_off < 0 || (a->gin_c_off % 8) != 0 || (a->gin_ld % 8) != 0 || a->gin_c_off + 256 > a->gin_ld))
        return fail(MAGNET_E_DIM, "magnet_gather_views: gin_ld=%lld gin_c_off=%d (multiples of 8, gin_c_off + 256 <= gin_ld)",
                    (long long)a->gin_ld, a->gin_c_off);
    if (!aligned16(a->pool_feat) || !aligned16(a->pool_xd3_hi) || !aligned16(a->pool_xd3_lo) || !aligned16(a->ref_cl) ||
        !aligned16(a->src_pad) || !aligned16(a->gin_hi) || !aligned16(a->gin_lo))
        return fail(MAGNET_E_ALIGN, "magnet_gather_views: features, x_d3 planes and their destinations must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(a->pool_gmm) | reinterpret_cast<uintptr_t>(a->ref_gmm) | reinterpret_cast<uintptr_t>(a->src_gmm) |
         reinterpret_cast<uintptr_t>(a->slots)) & 3u)
        return fail(MAGNET_E_ALIGN, "magnet_gather_views: slots and the (mu, sigma) tensors must be 4-byte aligned");
    hipError_t e = magnet::launch_gather_views(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_gather_views launch");
}

MAGNET_API int magnet_scatter_frames(const MagnetScatterFramesArgs* a, void* stream) {
    if (!a || !a->slots) return fail(MAGNET_E_NULL, "magnet_scatter_frames: NULL pointer");
    if (a->feat && !a->pool_feat) return fail(MAGNET_E_NULL, "magnet_scatter_frames: feat needs pool_feat");
    if (a->gmm && !a->pool_gmm) return fail(MAGNET_E_NULL, "magnet_scatter_frames: gmm needs pool_gmm");
    if ((a->xd3_hi != nullptr) != (a->xd3_lo != nullptr))
        return fail(MAGNET_E_DIM, "magnet_scatter_frames: xd3_hi and xd3_lo go together");
    if (a->xd3_hi && (!a->pool_xd3_hi || !a->pool_xd3_lo))
        return fail(MAGNET_E_NULL, "magnet_scatter_frames: the x_d3 planes need both x_d3 pool planes");
    if (a->feat_dtype != MAGNET_FEAT_F32 && a->feat_dtype != MAGNET_FEAT_BF16)
        return fail(MAGNET_E_DTYPE, "magnet_scatter_frames: unknown dtype %d", a->feat_dtype);
    const long long R = ((long long)a->h + 2) * ((long long)a->w + 2);
    if (a->n_slots <= 0 || a->n <= 0 || a->h <= 0 || a->w <= 0 || a->F <= 0 || (a->F % 8) != 0 || 2LL * a->n > 0x7fffffffLL ||
        R * 32 > 0x7fffffffLL || R * a->F / 4 > 0x7fffffffLL)
        return fail(MAGNET_E_DIM, "magnet_scatter_frames: bad dims n_slots=%d n=%d h=%d w=%d F=%d (F must be a multiple of 8)",
                    a->n_slots, a->n, a->h, a->w, a->F);
    if (!aligned16(a->feat) || !aligned16(a->xd3_hi) || !aligned16(a->xd3_lo) || !aligned16(a->pool_feat) ||
        !aligned16(a->pool_xd3_hi) || !aligned16(a->pool_xd3_lo))
        return fail(MAGNET_E_ALIGN, "magnet_scatter_frames: features, x_d3 planes and their pool tensors must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(a->gmm) | reinterpret_cast<uintptr_t>(a->pool_gmm) | reinterpret_cast<uintptr_t>(a->slots)) & 3u)
        return fail(MAGNET_E_ALIGN, "magnet_scatter_frames: slots and the (mu, sigma) tensors must be 4-byte aligned");
    hipError_t e = magnet::launch_scatter_frames(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_scatter_frames launch");
}

// PIL's coefficient row length for a pass from `in` to `out` pixels: 2 * ceil(max(in / out, 1)) + 1
static int image_prep_taps(int in, int out) { return 2 * (in > out ? (in + out - 1) / out : 1) + 1; }

// ---- frame preparation (image_prep.hip, depth_prep.hip): what the three entry points check alike ----
// The frames of N x Hin x Win pixels of `px` units (bytes or elements) each, their crop box, their pitches, and the size Hres x Wres
// the crop box is resized to.
static int prep_frames_check(const char* who, int N, int Hin, int Win, int Hres, int Wres, int left, int top, int cw, int ch,
                             long long pitch, long long frame, int px) {
    const int lim = 32768;
    if (N <= 0 || N > 65535 || Hin <= 0 || Win <= 0 || Hres <= 0 || Wres <= 0 || Hin > lim || Win > lim || Hres > lim || Wres > lim)
        return fail(MAGNET_E_DIM, "%s: bad dims N=%d Hin=%d Win=%d resized to H=%d W=%d (N <= 65535, sizes in [1, %d])", who, N, Hin, Win, Hres,
                    Wres, lim);
    if (left < 0 || top < 0 || cw <= 0 || ch <= 0 || left > Win - cw || top > Hin - ch)
        return fail(MAGNET_E_DIM, "%s: crop box left=%d top=%d %d x %d is not inside the %d x %d frame", who, left, top, cw, ch, Win, Hin);
    if (pitch < (long long)px * Win || (N > 1 && frame < pitch * Hin))
        return fail(MAGNET_E_DIM, "%s: src_pitch=%lld src_frame=%lld do not hold a row of %d pixels / a frame of %d rows", who, pitch, frame,
                    Win, Hin);
    return 0;
}

// The window of the training forms inside the resized image.
static int prep_window_check(const char* who, int Hres, int Wres, int Hout, int Wout) {
    if (Hout <= 0 || Wout <= 0 || Hout > Hres || Wout > Wres)
        return fail(MAGNET_E_DIM, "%s: the window %d x %d is not inside the resized %d x %d image", who, Wout, Hout, Wres, Hres);
    return 0;
}

// The two BILINEAR passes crop_w -> Wres and crop_h -> Hres: tap counts within the kernel's limit, tables exactly for a pass that
// resizes, row lengths what the sizes imply.
static int prep_passes_check(const char* who, int cw, int ch, int Hres, int Wres, const int32_t* coef_x, const int32_t* bounds_x,
                             const int32_t* coef_y, const int32_t* bounds_y, int akx, int aky) {
    const bool horiz = cw != Wres, vert = ch != Hres;
    const int kx = image_prep_taps(cw, Wres), ky = image_prep_taps(ch, Hres);
    if ((horiz && kx > MAGNET_IMAGE_PREP_KMAX) || (vert && ky > MAGNET_IMAGE_PREP_KMAX))
        return fail(MAGNET_E_SHAPE, "%s: %d x %d -> %d x %d needs %d x %d taps, MAGNET_IMAGE_PREP_KMAX is %d per axis "
                    "(downscale ratios up to %d)", who, cw, ch, Wres, Hres, horiz ? kx : 0, vert ? ky : 0,
                    MAGNET_IMAGE_PREP_KMAX, (MAGNET_IMAGE_PREP_KMAX - 1) / 2);
    if ((horiz && (!coef_x || !bounds_x)) || (vert && (!coef_y || !bounds_y)))
        return fail(MAGNET_E_NULL, "%s: a pass that resizes needs its coef and bounds tables", who);
    if ((horiz && akx != kx) || (vert && aky != ky))
        return fail(MAGNET_E_DIM, "%s: kx=%d ky=%d, the sizes imply rows of %d and %d taps", who, akx, aky, horiz ? kx : 0, vert ? ky : 0);
    return 0;
}

static bool aligned4(std::initializer_list<const void*> ps) {
    uintptr_t bits = 0;
    for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 3u) == 0;
}

MAGNET_API int magnet_image_prep_u8(const MagnetImagePrepArgs* a, void* stream) {
    const char* who = "magnet_image_prep_u8";
    if (!a || !a->src || !a->lut || !a->out) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (int r = prep_frames_check(who, a->N, a->Hin, a->Win, a->Hout, a->Wout, a->crop_left, a->crop_top, a->crop_w, a->crop_h,
                                  a->src_pitch, a->src_frame, 3)) return r;
    if (int r = prep_passes_check(who, a->crop_w, a->crop_h, a->Hout, a->Wout, a->coef_x, a->bounds_x, a->coef_y, a->bounds_y, a->kx, a->ky))
        return r;
    if (!aligned4({a->coef_x, a->bounds_x, a->coef_y, a->bounds_y, a->lut, a->out}))
        return fail(MAGNET_E_ALIGN, "%s: the tables and out must be 4-byte aligned", who);
    hipError_t e = magnet::launch_image_prep(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_image_prep_u8 launch");
}

MAGNET_API int magnet_train_prep_u8(const MagnetTrainPrepArgs* a, void* stream) {
    const char* who = "magnet_train_prep_u8";
    if (!a || !a->src || !a->luts || !a->frame_params || !a->out) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (int r = prep_frames_check(who, a->N, a->Hin, a->Win, a->Hres, a->Wres, a->crop_left, a->crop_top, a->crop_w, a->crop_h,
                                  a->src_pitch, a->src_frame, 3)) return r;
    if (int r = prep_window_check(who, a->Hres, a->Wres, a->Hout, a->Wout)) return r;
    if (a->n_luts < 1) return fail(MAGNET_E_DIM, "%s: n_luts=%d, at least one table is needed", who, a->n_luts);
    if (int r = prep_passes_check(who, a->crop_w, a->crop_h, a->Hres, a->Wres, a->coef_x, a->bounds_x, a->coef_y, a->bounds_y, a->kx, a->ky))
        return r;
    if (!aligned4({a->coef_x, a->bounds_x, a->coef_y, a->bounds_y, a->luts, a->frame_params, a->out}))
        return fail(MAGNET_E_ALIGN, "%s: the tables, frame_params and out must be 4-byte aligned", who);
    hipError_t e = magnet::launch_train_prep(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_train_prep_u8 launch");
}

MAGNET_API int magnet_depth_prep_u16(const MagnetDepthPrepArgs* a, void* stream) {
    const char* who = "magnet_depth_prep_u16";
    if (!a || !a->src || !a->frame_params || !a->out) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (int r = prep_frames_check(who, a->N, a->Hin, a->Win, a->Hres, a->Wres, a->crop_left, a->crop_top, a->crop_w, a->crop_h,
                                  a->src_pitch, a->src_frame, 1)) return r;
    if (int r = prep_window_check(who, a->Hres, a->Wres, a->Hout, a->Wout)) return r;
    if (!(a->divisor > 0.0f) || !__builtin_isfinite(a->divisor))
        return fail(MAGNET_E_DIM, "%s: divisor=%g must be finite and positive", who, (double)a->divisor);
    if ((a->idx_x == nullptr) != (a->crop_w == a->Wres) || (a->idx_y == nullptr) != (a->crop_h == a->Hres))
        return fail(MAGNET_E_NULL, "%s: %d x %d -> %d x %d takes an index table exactly for an axis that is resized", who, a->crop_w,
                    a->crop_h, a->Wres, a->Hres);
    if (!aligned4({a->idx_x, a->idx_y, a->frame_params, a->out}) || (reinterpret_cast<uintptr_t>(a->src) & 1u))
        return fail(MAGNET_E_ALIGN, "%s: the tables, frame_params and out must be 4-byte aligned, src 2-byte aligned", who);
    hipError_t e = magnet::launch_depth_prep(*a, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_depth_prep_u16 launch");
}

// ---- the D-Net's encoder (enc_kernels.hip) ----
// Each of the stem, the depthwise convolution and the scale has two entry points (`who`): the (hi, lo) form and the `_f16` form on ONE
// fp16 plane per grid (f16: the lo pointers do not exist there).  The checks are stated once.
static int enc_stem_run(const char* who, bool f16, const float* img, const float* wgt, const float* bias, void* out_hi, void* out_lo, int32_t N,
                        int32_t H, int32_t W, void* stream) {
    if (!img || !wgt || !bias || !out_hi || (!f16 && !out_lo)) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (N <= 0 || H < 2 || W < 2 || (int64_t)N * ((H + 1) / 2 + 2) * ((W + 1) / 2 + 2) >= ((int64_t)1 << 31))
        return fail(MAGNET_E_DIM, "%s: bad dims N=%d H=%d W=%d", who, N, H, W);
    if (!aligned16(out_hi) || !aligned16(out_lo)) return fail(MAGNET_E_ALIGN, "%s: outputs not 16-byte aligned", who);
    const hipError_t e = magnet::launch_enc_stem(img, wgt, bias, (uint16_t*)out_hi, (uint16_t*)out_lo, N, H, W, f16, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, f16 ? "magnet_enc_stem_f16 launch" : "magnet_enc_stem launch");
}

MAGNET_API int magnet_enc_stem(const float* img, const float* wgt, const float* bias, void* out_hi, void* out_lo, int32_t N, int32_t H, int32_t W,
                               void* stream) {
    return enc_stem_run("magnet_enc_stem", false, img, wgt, bias, out_hi, out_lo, N, H, W, stream);
}
MAGNET_API int magnet_enc_stem_f16(const float* img, const float* wgt, const float* bias, void* out_f16, int32_t N, int32_t H, int32_t W, void* stream) {
    return enc_stem_run("magnet_enc_stem_f16", true, img, wgt, bias, out_f16, nullptr, N, H, W, stream);
}

MAGNET_API int64_t magnet_dwconv_cl_parts(int32_t ho, int32_t wo) { return (ho <= 0 || wo <= 0) ? 0 : (int64_t)magnet::enc_dw_parts(ho, wo); }

static int dwconv_cl_run(const char* who, bool f16, const MagnetDwConvArgs* a, void* stream) {
    if (!a) return fail(MAGNET_E_NULL, "%s: args is NULL", who);
    if (!a->in_hi || (!f16 && !a->in_lo) || !a->wgt || !a->bias || !a->out_hi || (!f16 && !a->out_lo) || !a->part) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (f16 && (a->in_lo || a->out_lo)) return fail(MAGNET_E_DIM, "%s: in_lo and out_lo must be NULL (every grid is ONE fp16 plane)", who);
    if (a->k != 3 && a->k != 5) return fail(MAGNET_E_DIM, "%s: k=%d (3 or 5)", who, a->k);
    if (a->stride != 1 && a->stride != 2) return fail(MAGNET_E_DIM, "%s: stride=%d (1 or 2)", who, a->stride);
    if (a->N <= 0 || a->N > 65535 || a->h <= 0 || a->w <= 0 || a->c_pad <= 0 || (a->c_pad % 32) != 0)
        return fail(MAGNET_E_DIM, "%s: bad dims N=%d h=%d w=%d c_pad=%d (c_pad %% 32 == 0, N <= 65535)", who, a->N, a->h, a->w, a->c_pad);
    if (a->in_ld < a->c_pad || (a->in_ld % 8) != 0 || a->out_ld < a->c_pad || (a->out_ld % 8) != 0)
        return fail(MAGNET_E_DIM, "%s: in_ld=%d / out_ld=%d must be >= c_pad and multiples of 8", who, a->in_ld, a->out_ld);
    if (a->pad_top < 0 || a->pad_top >= a->k || a->pad_left < 0 || a->pad_left >= a->k)
        return fail(MAGNET_E_DIM, "%s: pad_top=%d pad_left=%d outside [0, k)", who, a->pad_top, a->pad_left);
    const int ho = (a->h + a->stride - 1) / a->stride, wo = (a->w + a->stride - 1) / a->stride;
    if ((int64_t)a->N * (a->h + 2) * (a->w + 2) >= ((int64_t)1 << 31)) return fail(MAGNET_E_DIM, "%s: N (h+2) (w+2) must be < 2^31", who);
    if (a->n_part != magnet::enc_dw_parts(ho, wo))
        return fail(MAGNET_E_DIM, "%s: n_part=%d, expected magnet_dwconv_cl_parts(%d, %d) = %lld", who, a->n_part, ho, wo, magnet::enc_dw_parts(ho, wo));
    if (!aligned16(a->in_hi) || !aligned16(a->in_lo) || !aligned16(a->out_hi) || !aligned16(a->out_lo) || !aligned16(a->wgt) || !aligned16(a->bias))
        return fail(MAGNET_E_ALIGN, "%s: planes, wgt and bias must be 16-byte aligned", who);
    if ((uintptr_t)a->part & 3) return fail(MAGNET_E_ALIGN, "%s: part must be 4-byte aligned", who);
    magnet::EncDwParams p;
    memset(&p, 0, sizeof(p));
    p.in_hi = (const uint16_t*)a->in_hi; p.in_lo = (const uint16_t*)a->in_lo; p.in_ld = a->in_ld; p.hi = a->h; p.wi = a->w; p.c_pad = a->c_pad;
    p.wgt = a->wgt; p.bias = a->bias; p.k = a->k; p.stride = a->stride; p.pad_top = a->pad_top; p.pad_left = a->pad_left;
    p.out_hi = (uint16_t*)a->out_hi; p.out_lo = (uint16_t*)a->out_lo; p.out_ld = a->out_ld; p.ho = ho; p.wo = wo; p.part = a->part;
    const hipError_t e = magnet::launch_enc_dwconv(p, a->N, f16, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, f16 ? "magnet_dwconv_cl_f16 launch" : "magnet_dwconv_cl launch");
}

MAGNET_API int magnet_dwconv_cl(const MagnetDwConvArgs* a, void* stream) { return dwconv_cl_run("magnet_dwconv_cl", false, a, stream); }
MAGNET_API int magnet_dwconv_cl_f16(const MagnetDwConvArgs* a, void* stream) { return dwconv_cl_run("magnet_dwconv_cl_f16", true, a, stream); }

MAGNET_API int magnet_se_gate(const float* part, int32_t n_part, int64_t hw, const float* w_reduce, const float* b_reduce, const float* w_expand_t,
                              const float* b_expand, int32_t C, int32_t R, int32_t c_pad, float* gate, int32_t N, void* stream) {
    if (!part || !w_reduce || !b_reduce || !w_expand_t || !b_expand || !gate) return fail(MAGNET_E_NULL, "magnet_se_gate: NULL pointer");
    if (N <= 0 || n_part <= 0 || hw <= 0 || hw >= ((int64_t)1 << 31) || C <= 0 || c_pad > 8192 || R <= 0 || R > 1024 || c_pad < C || (c_pad % 32) != 0)
        return fail(MAGNET_E_DIM, "magnet_se_gate: bad dims N=%d n_part=%d hw=%lld C=%d R=%d c_pad=%d (C <= c_pad <= 8192, R <= 1024, c_pad %% 32 == 0)", N,
                    n_part, (long long)hw, C, R, c_pad);
    if (!aligned16(part) || ((uintptr_t)gate & 3)) return fail(MAGNET_E_ALIGN, "magnet_se_gate: part must be 16-byte aligned, gate 4-byte aligned");
    const hipError_t e = magnet::launch_enc_se_gate(part, n_part, hw, w_reduce, b_reduce, w_expand_t, b_expand, C, R, c_pad, gate, N, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "magnet_se_gate launch");
}

static int se_scale_run(const char* who, bool f16, const void* in_hi, const void* in_lo, int32_t in_ld, const float* gate, int32_t N, int32_t h, int32_t w,
                        int32_t c_pad, void* out_hi, void* out_lo, int32_t out_ld, void* stream) {
    if (!in_hi || (!f16 && !in_lo) || !gate || !out_hi || (!f16 && !out_lo)) return fail(MAGNET_E_NULL, "%s: NULL pointer", who);
    if (N <= 0 || h <= 0 || w <= 0 || c_pad <= 0 || (c_pad % 32) != 0 || in_ld < c_pad || (in_ld % 8) != 0 || out_ld < c_pad || (out_ld % 8) != 0 ||
        (int64_t)N * (h + 2) * (w + 2) >= ((int64_t)1 << 31))
        return fail(MAGNET_E_DIM, "%s: bad dims N=%d h=%d w=%d c_pad=%d in_ld=%d out_ld=%d (c_pad %% 32 == 0; pitches >= c_pad, multiples of 8)", who, N, h,
                    w, c_pad, in_ld, out_ld);
    if (!aligned16(in_hi) || !aligned16(in_lo) || !aligned16(out_hi) || !aligned16(out_lo) || !aligned16(gate))
        return fail(MAGNET_E_ALIGN, "%s: planes and gate must be 16-byte aligned", who);
    const hipError_t e = magnet::launch_enc_se_scale((const uint16_t*)in_hi, (const uint16_t*)in_lo, in_ld, gate, N, h, w, c_pad, (uint16_t*)out_hi,
                                                     (uint16_t*)out_lo, out_ld, f16, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, f16 ? "magnet_se_scale_f16 launch" : "magnet_se_scale launch");
}

MAGNET_API int magnet_se_scale(const void* in_hi, const void* in_lo, int32_t in_ld, const float* gate, int32_t N, int32_t h, int32_t w, int32_t c_pad,
                               void* out_hi, void* out_lo, int32_t out_ld, void* stream) {
    return se_scale_run("magnet_se_scale", false, in_hi, in_lo, in_ld, gate, N, h, w, c_pad, out_hi, out_lo, out_ld, stream);
}
MAGNET_API int magnet_se_scale_f16(const void* in_f16, int32_t in_ld, const float* gate, int32_t N, int32_t h, int32_t w, int32_t c_pad, void* out_f16,
                                   int32_t out_ld, void* stream) {
    return se_scale_run("magnet_se_scale_f16", true, in_f16, nullptr, in_ld, gate, N, h, w, c_pad, out_f16, nullptr, out_ld, stream);
}

}  // extern "C"
