/*
 * magnet_hip.h — C ABI of libmagnet_hip.so, the MI355X (gfx950) implementation of MaGNet's
 * multi-view matching hot path.  Plain pointers and sizes only; no torch types.  Every entry
 * point replaces a specific piece of the reference (file:line into baegwangbin/MaGNet):
 *
 *   magnet_pack_features     -> the layout hand-off from F-Net's NCHW fp32 output
 *                               (models/MAGNET.py:142-144) to the kernel's channel-last storage
 *   magnet_pack_gmm          -> the same for D-Net's source-view (mu,sigma) maps (models/MAGNET.py:139)
 *   magnet_cost_volume_cw    -> homography.est_costvolume_CW  (models/submodules/homography.py:79-121)
 *                               + _compute_cost_CW            (homography.py:124-161)
 *                               + the candidate sampling in front of it (models/MAGNET.py:153-156)
 *   magnet_gaussian_update   -> the element-wise tail of GNET.forward (models/MAGNET.py:60-69)
 *   magnet_upsample_depth    -> upsample_depth_via_mask       (models/MAGNET.py:15-27)
 *   magnet_depth_metrics     -> utils.compute_depth_errors + validate()'s masking (utils/utils.py:106-144,
 *                               test_MaGNet.py:43,58-79), so full depth maps never leave the device
 *   magnet_conv_mfma (+ magnet_pack_split, magnet_gaussian_update_cl, magnet_upsample_depth_cl[_n])
 *                            -> the g_net / mask_head nn.Conv2d stacks (models/MAGNET.py:51-56,111-116)
 *
 * Conventions
 *   - All data pointers are DEVICE pointers unless the comment says HOST.  Buffers are caller-owned;
 *     the library never synchronises the device and keeps no device memory between calls.  ONE exception to
 *     "never allocates": magnet_depth_metrics / magnet_depth_metrics_crop take their B x 64 x 13 doubles of
 *     partial sums from the stream-ordered pool (hipMallocAsync + hipFreeAsync on `stream`, inside the call);
 *     every other entry point works in caller-provided buffers only (magnet_depth_metrics_ex is the same reduction in a caller's
 *     work buffer).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous on that stream and re-entrant across streams.
 *   - Return value: 0 on success; >0 = MAGNET_E_* argument error; <0 = -(hipError_t).  Nothing is
 *     thrown.  magnet_last_error() returns a thread-local message for the last failing call.
 *   - Layouts follow the reference: NCHW fp32 for (mu,sigma) maps and the cost volume, source-view
 *     tensors VIEW-MAJOR (index v*B + b, homography.py:105), rays (B,3,h*w), intM (B,3,3),
 *     poses (B,V,4,4) row-major [R|t], is_valid (B,V) int32 (1 = use the view, homography.py:97).
 */
#ifndef MAGNET_HIP_H
#define MAGNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAGNET_API __attribute__((visibility("default")))

#define MAGNET_HIP_VERSION 500            /* major*10000 + minor*100 + patch.
                                           * BINARY COMPATIBILITY: the argument structs below carry no size field and have grown at their END between versions
                                           * (MagnetConvArgs: v300 up_*, v301 gu_*).  A caller must be compiled against the header whose
                                           * MAGNET_HIP_VERSION equals magnet_version() of the library it loads, and must check that at load time (INTEGRATION.md;
                                           * magnet_amd/lib.py mirrors the structs field for field and tests/test_abi.py compares the layouts with a gcc probe).
                                           * From v400 on a struct change bumps the MINOR number, never only the patch.
                                           * v500 REMOVED the v302 fp16 + block-scaled e4m3 operand format (the last three fields of MagnetConvArgs and its
                                           * pack entry point) and magnet_conv1x1_chain: MagnetConvArgs, and with it every struct that embeds it, is shorter.
                                           * Added since, with no struct change and therefore under the same number: magnet_conv_mfma_f16e,
                                           * magnet_enc_stem_f16, magnet_dwconv_cl_f16, magnet_se_scale_f16 (the encoder's fp16 single-plane mode);
                                           * magnet_image_prep_u8 with its own new MagnetImagePrepArgs (uint8 camera frames to the backbones' input);
                                           * magnet_train_prep_u8 and magnet_depth_prep_u16 with their own new MagnetTrainPrepArgs and MagnetDepthPrepArgs
                                           * (training samples: the same resize with a per-frame flip, crop window and augmentation table; ground-truth depth). */

enum {                                     /* storage dtype of channel-last feature maps */
    MAGNET_FEAT_F32  = 0,
    MAGNET_FEAT_BF16 = 1
};

enum {                                     /* argument errors (positive return values) */
    MAGNET_E_NULL     = 1,                 /* a required pointer is NULL */
    MAGNET_E_DIM      = 2,                 /* a dimension is <= 0 or exceeds a kernel limit */
    MAGNET_E_DTYPE    = 3,                 /* unknown dtype enum */
    MAGNET_E_ALIGN    = 4,                 /* a pointer is not 16-byte aligned */
    MAGNET_E_NODEVICE = 5,                 /* no gfx950 device / kernel image not loadable */
    MAGNET_E_SHAPE    = 6                  /* valid arguments, but the kernel selected by `path` (or the requested output form)
                                              does not take this shape / option set: choose another path.  Never a HIP failure. */
};

#define MAGNET_MAX_CANDIDATES 256          /* D limit of magnet_cost_volume_cw */

/* Arguments of magnet_cost_volume_cw.  Zero-initialise, then fill. */
typedef struct MagnetCostVolumeArgs {
    int32_t B, V, F, D, h, w;              /* ref frames, source views, channels (F % 8 == 0), candidates, grid */
    float   kappa;                         /* consistency threshold: int(weighting.split('CW')[1]), MAGNET.py:159 */
    int32_t feat_dtype;                    /* MAGNET_FEAT_* of ref_feat_cl / src_feat_cl */
    const void    *ref_feat_cl;            /* (B, h, w, F) channel-last            (magnet_pack_features, pad = 0) */
    const void    *src_feat_pad;           /* (V*B, h+2, w+2, F) channel-last with a one-texel ZERO border, view-major
                                              (magnet_pack_features, pad = 1): grid_sample's zeros padding
                                              (homography.py:150) becomes plain loads */
    const float   *src_gmm_pad;            /* (V*B, h+2, w+2, 2) interleaved source [mu, sigma], zero border
                                              (magnet_pack_gmm).  May be NULL when src_gmm_quad is given: a call that ends up in a
                                              kernel that reads this layout then returns MAGNET_E_SHAPE */
    const float   *ref_gmm;                /* (B, 2, h, w) reference [mu, sigma]; used when d_volume == NULL */
    const double  *k_list;                 /* HOST, D float64 quantile offsets (MAGNET.depth_sampling, MAGNET.py:120-128);
                                              used when d_volume == NULL: d_j = mu + sigma*(float)k_j */
    const float   *d_volume;               /* optional (B,D,h,w) explicit candidate depths (the reference's first
                                              argument); NULL = fused sampling from ref_gmm + k_list */
    const float   *poses;                  /* (B,V,4,4) relative poses ref->source (utils.data_preprocess) */
    const int32_t *is_valid;               /* (B,V) */
    const float   *intM;                   /* (B,3,3) intrinsics at grid resolution */
    const float   *rays;                   /* (B,3,h*w) unit_ray_array_2D; may be NULL when ray_params is given (path 0/1/2/4) */
    float         *cost;                   /* OUT (B,D,h,w) fp32; frame b starts at cost + b*cost_batch_stride */
    int32_t        path;                   /* kernel selection:
                                              0 = auto: the PRODUCTION matcher whenever the candidates are sampled in the kernel
                                                  (d_volume == NULL, mode 0, stats == NULL); otherwise the exact candidate-lane
                                                  kernel; the generic kernel for shapes neither takes.
                                                  Production contract (TOLERANCE parity with homography.py:124-161): at most a 1e-5 x
                                                  max(1, (max(h, w) + 1) / 161) fraction of the consistency gates differs from the
                                                  reference's (1e-5 up to 160-wide grids; measured 1.2e-5 at the 640-wide C2L grid: both
                                                  sides' positions carry ~ulp(max(h, w)) texels of fp32 rounding); every entry none
                                                  of whose gates differs is within 2e-5 + 2e-5|c| + eps*S of the reference, where
                                                  S = sum over open views of (|dc/dx| + |dc/dy|) is the score's slope in the sample
                                                  position and eps = 4 ulp(max(h, w) + 1) texels (6 ulp on grids wider than 512): the kernel's sample position
                                                  differs from the reference's by its normalise / unnormalise rounding (<= 1.5e-5
                                                  texel), so on features that vary strongly from texel to texel (white noise) the
                                                  plain 2e-5 + 2e-5|c| bound alone does NOT hold; on smooth features it does
                                                  (tests/test_gpu_fast_matcher.py).  Downstream of the volume, north_star's bar — depth abs_rel
                                                  < 1e-4 against the reference loop — holds with a measured worst case of 2.2e-5 (C3 shape,
                                                  bf16 feature storage, I = 3, production matcher + matrix-core convolutions against the
                                                  oracle loop; 8e-8 .. 2.8e-7 against the reference's own forward on its fixtures G6 / G13);
                                              1 = generic gather kernel (bit-exact reference arithmetic, slow);
                                              2 = exact candidate-lane kernel (the reference's fp32 geometry to the bit) or MAGNET_E_SHAPE;
                                              3 = exact pixel-lane worklist kernel or MAGNET_E_SHAPE;
                                              4 = production matcher or MAGNET_E_SHAPE.
                                              Any other value: MAGNET_E_DIM. */
    uint32_t      *stats;                  /* optional device uint32[4]: {tiles run by a fast kernel, tiles run by the
                                              generic kernel, items (distinct open quads) correlated, 0}, accumulated with atomics; NULL = off */
    int64_t        cost_batch_stride;      /* elements between consecutive frames of `cost`; 0 = D*h*w (dense).
                                              Lets the kernel write the first D channels of G-Net's
                                              (B, D+256, h, w) input directly (models/MAGNET.py:167). */
    void          *cost_hi, *cost_lo;      /* optional second output form (candidate-lane kernel only): the cost volume as
                                              split-bf16 planes (hi = bf16(c), lo = bf16(c - hi)) in the conv kernel's
                                              zero-bordered channel-last layout, element [((b*(h+2)+y+1)*(w+2)+x+1)*cost_ld + j].
                                              When set, `cost` may be NULL (nothing is written there). */
    int64_t        cost_ld;                /* row pitch (elements) of cost_hi / cost_lo */
    int32_t        mode;                   /* 0 = consistency-weighted matcher (est_costvolume_CW);
                                              1 = plain feature-matching volume of est_costvolume_F / _compute_cost_F
                                                  (homography.py:10-75) BEFORE its softmax: k_list holds the D fixed depth
                                                  bins d_center (same for all pixels), there is no gate (src_gmm_pad,
                                                  ref_gmm unused, may be NULL) and views are summed in fp32 (:42).
                                                  Candidate-lane and generic kernels only. */
    uint8_t       *gate_bits;              /* optional debug OUT (B,V,D,h,w) uint8: the consistency gate of every
                                              (view, candidate, pixel) sample, homography.py:157-158 (1 = open).  Written by the
                                              production matcher (path 0/4) and by the exact candidate-lane kernel (path 2);
                                              entries of invalid views are not written (zero the buffer first).  NULL = off. */
    const double  *ray_params;             /* optional DEVICE (B,8) float64 {fx, fy, cx, cy, sx, sy, left, top} of the RAW image
                                              (sx = raw_w / w, sy = raw_h / h; left/top = crop margins, KITTI): with rays == NULL the
                                              production and candidate-lane / generic kernels evaluate the loaders' expression
                                              ((x+0.5)*sx - cx + left)/fx in float64 per reference pixel instead of reading the
                                              12*h*w-byte table (dataloader_scannet.py:139-147, dataloader_kitti.py:113-118) —
                                              bit-identical to it.  The worklist kernel and the backward need the table. */
    const float   *src_gmm_quad;           /* optional (V*B, h+2, w+2, 8): the source (mu, sigma) map per QUAD ORIGIN of the padded map in
                                              quad form {m00, m10-m00, m01-m00, m11-m10-m01+m00, s00, ...} (magnet_pack_gmm_quad), so that
                                              a bilinear sample is 3 fma per channel.  The production matcher for D > 32 needs it
                                              (without it path 0 runs the round-2 production kernel, path 4 too). */
    uint32_t       dev_flags;              /* development switches (timing ablations, kernel variants of tools/ablate.py).  Ignored
                                              unless the library was built with -DMAGNET_DEV (python -m magnet_amd.build --dev);
                                              results are not meaningful with any of them set. */
} MagnetCostVolumeArgs;

MAGNET_API int magnet_version(void);
MAGNET_API const char *magnet_last_error(void);

/* Number of gfx950 devices visible to the HIP runtime this library is bound to (0 if none). */
MAGNET_API int magnet_device_count(void);

/* NCHW fp32 (N,F,h,w) -> channel-last (N,h+2*pad,w+2*pad,F) in `out_dtype` (round-to-nearest-even for
 * bf16); pad = 1 surrounds every image with one texel of zeros. */
MAGNET_API int magnet_pack_features(const float *nchw, void *out_cl, int32_t N, int32_t F, int32_t h, int32_t w,
                         int32_t out_dtype, int32_t pad, void *stream);

/* (N,2,h,w) fp32 [mu,sigma] planes -> (N,h+2,w+2,2) interleaved with a one-texel zero border. */
MAGNET_API int magnet_pack_gmm(const float *gmm_nchw, float *out_pad, int32_t N, int32_t h, int32_t w, void *stream);

/* (N,2,h,w) fp32 [mu,sigma] planes -> (N,h+2,w+2,8): entry (y0,x0) describes the 2x2 quad of the zero-bordered map whose top-left
 * texel is padded position (y0,x0) (texels outside the padded map count as zero), as
 * {m00, m10-m00, m01-m00, (m11-m01)-(m10-m00), s00, s10-s00, s01-s00, (s11-s01)-(s10-s00)} (x is the fast index of mXY).
 * Feeds MagnetCostVolumeArgs.src_gmm_quad (grid_sample of the (mu, sigma) maps, homography.py:151-152). */
MAGNET_API int magnet_pack_gmm_quad(const float *gmm_nchw, float *out_quad, int32_t N, int32_t h, int32_t w, void *stream);

/* Consistency-weighted multi-view matching score, all (b, pixel, candidate) in one launch. */
MAGNET_API int magnet_cost_volume_cw(const MagnetCostVolumeArgs *args, void *stream);

/* Backward of mode 1 (what autograd derives for est_costvolume_F up to its softmax, homography.py:10-75,
 * used by train_scripts/train_FNET/train.py): given grad_cost (B,D,h,w) = dL/d(cost before softmax) and
 * the SAME args as the forward call (fp32 features, mode = 1; `cost` is ignored),
 *   grad_ref_cl  (B,h,w,F)         fp32 channel-last, fully written;
 *   grad_src_pad (V*B,h+2,w+2,F)   fp32 padded channel-last, ACCUMULATED into with atomics — zero it first;
 *                                  what lands in the one-texel border is the (discarded) gradient of the
 *                                  zero padding.
 * Depth bins, poses and intrinsics receive no gradient (they are data in the reference's training loop).
 * Limits (MAGNET_E_DIM otherwise, outputs untouched): V <= 29 (the per-wave projection table, 4 * (512 V + 1360) bytes, must fit
 * 64 KB of LDS); F <= 128, or any F % 32 == 0 while V <= 4 (the LDS hash kernel walks the channels in slices of 32). */
MAGNET_API int magnet_cost_volume_f_backward(const MagnetCostVolumeArgs *args, const float *grad_cost, float *grad_ref_cl,
                                  float *grad_src_pad, void *stream);

/* ---- camera intrinsics and relative poses on the device (the loaders' / utils.data_preprocess' host work; row N4) ----
 * magnet_make_rays: unit_ray_array_2D (B,3,h*w) fp32 from DEVICE ray_params (B,8) float64 {fx, fy, cx, cy, sx, sy, left, top}
 *   (see MagnetCostVolumeArgs.ray_params; data/dataloader_scannet.py:113-153, dataloader_kitti.py:83-127, dataloader_7scenes.py:72-116).
 * magnet_relative_poses: utils.data_preprocess (utils/utils.py:72-98): DEVICE float64 extrinsics ext_ref (B,4,4), ext_nghbr
 *   (B,V,4,4) -> poses_out (B,V,4,4) fp32 = ext_nghbr @ inv(ext_ref) and is_valid_out (B,V) int32 (0 and a zero pose when either
 *   matrix holds a NaN or the reference is singular).  Both outputs are what magnet_cost_volume_cw consumes. */
MAGNET_API int magnet_make_rays(const double *ray_params, float *rays_out, int32_t B, int32_t h, int32_t w, void *stream);
MAGNET_API int magnet_relative_poses(const double *ext_ref, const double *ext_nghbr, float *poses_out, int32_t *is_valid_out,
                                     int32_t B, int32_t V, void *stream);

/* The same backward with a caller-provided device workspace of magnet_cost_volume_f_backward_workspace(args) bytes: grad_src is then
 * computed as a GATHER per source row segment (cost_volume_f_gather.hip) — no atomics, deterministic, every interior texel of
 * grad_src_pad stored exactly once (the one-texel border is left as the caller initialised it) — and grad_ref by the per-item
 * kernel.  Shapes the gather path does not take fall back to the scatter kernels above (which accumulate: zero grad_src_pad
 * first to be safe).  The workspace query returns -1 for invalid arguments. */
MAGNET_API int64_t magnet_cost_volume_f_backward_workspace(const MagnetCostVolumeArgs *args);
MAGNET_API int magnet_cost_volume_f_backward_ws(const MagnetCostVolumeArgs *args, const float *grad_cost, float *grad_ref_cl,
                                     float *grad_src_pad, void *workspace, int64_t workspace_bytes, void *stream);

/* gmm_out[:,0] = mu + o0*sigma ; gmm_out[:,1] = (elu(o1) + 1 + 1e-10)*sigma.   All (B,2,h*w) fp32.
 * gmm_out may alias gmm_in. */
MAGNET_API int magnet_gaussian_update(const float *gnet_out, const float *gmm_in, float *gmm_out,
                           int32_t B, int32_t hw, void *stream);

/* Learned convex upsampling: depth (B,C,h,w), mask (B,9*k*k,h,w) -> out (B,C,k*h,k*w); softmax over
 * the 9 neighbours, zero padding.  k <= 8. */
MAGNET_API int magnet_upsample_depth(const float *depth, const float *mask, float *out,
                          int32_t B, int32_t C, int32_t h, int32_t w, int32_t k, void *stream);

/* ---- G-Net / mask-head convolutions on the bf16 matrix cores, bf16x3 split operands (fp32-grade) ----
 * Replaces the nn.Conv2d stacks of models/MAGNET.py:51-56 (GNET.gnet) and :111-116 (mask_head).
 * Activations live in ZERO-BORDERED channel-last buffers (B, h+2, w+2, C) stored as two bf16 planes
 * (hi = bf16(x), lo = bf16(x - hi)); `rows` = B*(h+2)*(w+2) flattened positions; a 3x3 tap is the row
 * offset dy*(w+2)+dx.  Border rows of the output hold unspecified finite values or are not written at all: read interior rows
 * only.  (Launches with gu_in or up_depth know their image geometry and tile each image on its own from its first interior image
 * row when that takes fewer workgroups: the top and bottom border image rows are then not computed.  MagnetConvExArgs.tiling.)
 * Weights: two bf16 planes of [taps][cout_pad][cin] (cin contiguous) — magnet_amd/convnet.py prepacks them
 * from nn.Conv2d's [cout][cin][kh][kw]; bias fp32 [cout_pad] (zero in the padding).
 * Limits: cin % 32 == 0; taps in {1, 4, 9}; cout_pad a multiple of 128, or 144, 64, 32, 16.
 * The same kernel runs the F-Net (PSMNet feature extractor, models/submodules/F_psmnet.py:37-124) — see the fields
 * after `addend_ld` (all zero = the behaviour described above). */
typedef struct MagnetConvArgs {
    const void  *in_hi, *in_lo;            /* bf16 (rows, cin) */
    const void  *w_hi, *w_lo;              /* bf16 (taps, cout_pad, cin) */
    const float *bias;                     /* (cout_pad) */
    void        *out_hi, *out_lo;          /* out_mode 0: bf16 (rows, cout_pad) planes */
    float       *out_f32;                  /* out_mode 1: fp32 (rows, cout_pad) */
    int64_t      rows;
    int32_t      cin, cout_pad, taps, wp;  /* wp = w + 2 (row pitch of the padded grid) */
    int32_t      relu, out_mode;
    int32_t      in_ld;                    /* elements between input rows (0 = cin): lets a layer read a channel slice
                                              of a wider buffer in place (pointer offset + in_ld) */
    const float *addend;                   /* optional fp32 (rows, addend_ld): added to the accumulator before bias / ReLU.
                                              Used to hoist the loop-invariant x_d3 part of G-Net's first layer out of
                                              the refinement loop (models/MAGNET.py:151-168): W*[cost|x_d3] = Wc*cost + Wx*x_d3.
                                              Excludes add_hi / add_lo: a launch has ONE pre-bias term (both: MAGNET_E_DIM) */
    int32_t      addend_ld;                /* row pitch of addend (0 = cout_pad) */
    int32_t      dil;                      /* taps = 9: dilation (0 or 1 = none); the grid's border must be >= dil wide
                                              (F_psmnet.py:47 layer4).  taps = 4: the 2x2 window (-1,-1),(-1,0),(0,-1),(0,0)
                                              of a space-to-depth tensor = a stride-2 3x3 convolution (F_psmnet.py:40,45) */
    int32_t      out_ld;                   /* elements between output rows (0 = cout_pad): write a channel slice of a wider
                                              buffer in place (the 320-channel concatenation, F_psmnet.py:122) */
    const void  *add_hi, *add_lo;          /* optional split-bf16 (rows, add_ld) residual input added before bias / ReLU
                                              (BasicBlock `out += x`, F_psmnet.py:27-33): hi + lo is formed in fp32 (exact: it is
                                              the fp32 value the planes were split from).  Excludes `addend` (both: MAGNET_E_DIM) */
    int32_t      add_ld;
    int32_t      border_hp;                /* > 0: rows are positions of (image, border_hp, wp) grids with a `border_pad`-wide
                                              border; outputs at border positions are written as ZEROS (they are the next
                                              layer's zero padding) */
    int32_t      border_pad;
    int32_t      repad;                    /* > 0 (needs border_hp): only interior positions are written, re-addressed into
                                              grids with a (repad-1)-wide border: hands the last layer's output to the
                                              matcher's layouts (border 0 = reference features, 1 = source features) */
    const void  *tail_w_hi, *tail_w_lo;    /* optional fused 1x1 tail (models/MAGNET.py:53-55, :113-115): after THIS layer (cout_pad
                                              must be 128; bias / relu / addend apply) the workgroup's 128-row tile stays in LDS and
                                              relu(1x1 128->128), relu(1x1 128->128), 1x1 128->tail_cout_pad run in the same kernel.
                                              Weights: the three layers' [cout][128] bf16 planes concatenated; bias: 128 + 128 +
                                              tail_cout_pad floats.  The only output is fp32
                                              (rows, tail_cout_pad) at out_f32 (out_mode, out_hi/lo, out_ld are ignored): the three
                                              hidden (rows,128) tensors never reach HBM. */
    const float *tail_bias;
    int32_t      tail_cout_pad;            /* 16, 128 or 144 */
    /* v301 — fused learned convex upsampling (models/MAGNET.py:15-27,172-173), for the mask head's stack (tail_cout_pad = 144):
     * the tail's last layer keeps the (rows, 144) mask logits in registers, soft-maxes the 9 neighbour weights of each of the 16
     * sub-pixels and writes the x4-upsampled maps itself: up_depth (up_npred, up_B, 2, up_h, up_w) fp32 -> up_out (up_npred, up_B,
     * 2, 4 up_h, 4 up_w) fp32.  Requires rows = up_B * (up_h + 2) * (up_w + 2), wp = up_w + 2; out_f32 is not written.
     * All zero / NULL = the plain tail above (magnet_upsample_depth_cl_n then does this step from out_f32). */
    const float *up_depth;
    float       *up_out;
    int32_t      up_npred, up_B, up_h, up_w;
    /* v301 — fused Gaussian update (models/MAGNET.py:60-69), for G-Net's stack (tail_cout_pad = 16): the head's two outputs of every
     * interior position update (mu, sigma): gu_in (up_B, 2, up_h, up_w) fp32 -> gu_out (same layout; may not alias gu_in); up_B /
     * up_h / up_w as above, out_f32 is not written.  NULL = plain tail (magnet_gaussian_update_cl then does this step). */
    const float *gu_in;
    float       *gu_out;
    /* `bias` is read with 16-byte loads in every format: 16-byte aligned, as all pointers of this struct. */
    /* The SINGLE-PLANE FP16 format (magnet_conv_mfma_f16 below; an entry point of its own, no field of this struct): in_hi is ONE fp16
     * plane (rows, in_ld), w_hi ONE fp16 plane (taps, cout_pad, cin); in_lo, w_lo are NULL.  The 3x3 layer issues one fp16
     * matrix instruction per product (each fp16 x fp16 product is exact in the fp32 accumulator) instead of three bf16 ones; the
     * operands carry 11 significant bits instead of 16.  It is a reduced-precision mode the caller opts into, not fp32-grade.
     * DOMAIN: |x| <= 65504; relative rounding 2^-11 for |x| >= 2^-14, absolute 2^-25 below (fp16 denormals are kept).  magnet_pack_f16 and
     * magnet_planes_to_f16 write the activation plane: round to nearest even, magnitudes that would round above 65504 (+-Inf included)
     * become +-65504 (never Inf), NaN is written through, the sign of zero is kept.  The fused 1x1 tail layers, bias, addend,
     * ReLU, the Gaussian update and the convex upsampling behind the 3x3 layer are those of the bf16x3 format (tail_w_hi / tail_w_lo stay
     * bf16 planes).
     * A SECOND entry point reads this format, magnet_conv_mfma_f16p ("plane to plane", the F-Net's layers): there the residual input
     * (add_hi) is one fp16 plane too and out_mode 3 writes the result as ONE fp16 plane at out_hi, converted exactly as
     * magnet_pack_f16 converts: every activation of a network then lives in this format from layer to layer.  Its domain is the
     * format's, |x| <= 65504, CLAMPED: a layer output beyond it (an un-ReLU'd residual sum, say) is stored as +-65504 and not as Inf; a
     * trained PSMNet's residual stream is bounded by its BatchNorms (seeded networks: below 10), but nothing checks it at run time.  NaN is written through. */
} MagnetConvArgs;                          /* out_mode 2: one bf16 plane (round-to-nearest-even) at out_hi */

MAGNET_API int magnet_conv_mfma(const MagnetConvArgs *args, void *stream);

/* ---- the F-Net's non-GEMM layers (PSMNet feature extractor, models/submodules/F_psmnet.py:37-124; row N3) ----
 * Activations are conv_mfma's format: zero-bordered channel-last grids as two bf16 planes (hi, lo). */

/* firstconv[0] (F_psmnet.py:40): 3x3 stride-2 pad-1 convolution 3 -> 32 channels of the NCHW fp32 image (N,3,H,W) with the
 * BatchNorm folded into wgt (32,3,3,3) / bias (32), then ReLU -> planes (N, H2+2, W2+2, 32), border 1 (interior written),
 * H2 = (H-1)/2+1, W2 = (W-1)/2+1. */
MAGNET_API int magnet_fnet_stem(const float *img, const float *wgt, const float *bias, void *out_hi, void *out_lo,
                                int32_t N, int32_t H, int32_t W, void *stream);

/* (N, H2+2, W2+2, C) border 1 -> (N, H4+2*opad, W4+2*opad, 4*C) border opad, channel (py*2+px)*C + c = in[2y+py, 2x+px, c]
 * (zero where 2y+py >= H2 or 2x+px >= W2); H4 = (H2-1)/2+1.  With it the stride-2 convolutions of layer2[0]
 * (F_psmnet.py:45,89-93) are stride-1 GEMMs: 3x3/s2 = conv_mfma taps=4 over 4*C channels, 1x1/s2 = taps=1 on phase 0.
 * C % 8 == 0; interior written only. */
MAGNET_API int magnet_space_to_depth(const void *in_hi, const void *in_lo, void *out_hi, void *out_lo, int32_t N, int32_t C,
                                     int32_t H2, int32_t W2, int32_t opad, void *stream);

/* AvgPool2d((k,k), stride (k,k)) (F_psmnet.py:50-64) of channels [0,C) at in_hi/in_lo (row pitch ld elements) of an
 * (N, h+2*pad, w+2*pad) grid -> planes (N*(h/k)*(w/k), C).  C <= 128, C % 8 == 0. */
MAGNET_API int magnet_avgpool_cl(const void *in_hi, const void *in_lo, int32_t ld, int32_t N, int32_t h, int32_t w, int32_t pad,
                                 int32_t k, int32_t C, void *out_hi, void *out_lo, void *stream);

/* F.interpolate(..., mode='bilinear', align_corners=True) (F_psmnet.py:108-119): fp32 (N*ph*pw, in_ld) -> planes, channels
 * [0,C) at out_hi/out_lo (row pitch out_ld) of an (N, h+2*pad, w+2*pad) grid, interior only.  C % 8 == 0. */
MAGNET_API int magnet_upsample_bilinear_cl(const float *in, int32_t in_ld, int32_t ph, int32_t pw, int32_t C, void *out_hi,
                                           void *out_lo, int32_t out_ld, int32_t N, int32_t h, int32_t w, int32_t pad,
                                           void *stream);

/* fp32 NCHW (N, C, h, w) (image stride `in_img_stride` elements, 0 = C*h*w) -> the interior of the split-bf16
 * padded channel-last buffer (N, h+2, w+2, ctot), channels [c_off, c_off+round_up(C,8)) (the round-up lanes are
 * written as zeros).  c_off % 8 == 0.  The border must have been zeroed once by the caller (never written).
 * CONTRACT: whole 8-channel vectors are stored, so with C % 8 != 0 the channels [c_off+C, c_off+round_up(C,8)) of every interior
 * position are OVERWRITTEN with +0 in both planes (C = 5: channels 5..7); a caller that packs several tensors side by side must
 * place each at a multiple of 8 and pack in ascending order or leave the gap unused (ConvStackMFMA's in_map relies on the zeros:
 * the first layer's weights are zero there, and 0 * 0 adds nothing).  No other element of the buffer is touched. */
MAGNET_API int magnet_pack_split(const float *nchw, void *out_hi, void *out_lo, int32_t N, int32_t C, int32_t h,
                                 int32_t w, int32_t ctot, int32_t c_off, int64_t in_img_stride, void *stream);

/* G-Net tail on the conv kernel's fp32 output: o = gnet_out[(b, y+1, x+1), 0..1] of a (B, h+2, w+2, ld) buffer;
 * gmm_out = [mu + o0*sigma, (elu(o1) + 1 + 1e-10)*sigma], all gmm tensors (B,2,h,w) fp32 (models/MAGNET.py:60-69). */
MAGNET_API int magnet_gaussian_update_cl(const float *gnet_out_pad, int32_t ld, const float *gmm_in, float *gmm_out,
                                         int32_t B, int32_t h, int32_t w, void *stream);

/* Learned convex upsampling with the mask in the conv kernel's padded channel-last fp32 layout
 * (B, h+2, w+2, ld), channel n*k*k + i*k + j as in models/MAGNET.py:19; depth (B,2,h,w) -> out (B,2,4h,4w); k = 4. */
MAGNET_API int magnet_upsample_depth_cl(const float *depth, const float *mask_pad, int32_t ld, float *out,
                                        int32_t B, int32_t h, int32_t w, void *stream);
/* The same for n_pred stacked predictions in one launch: depths (n_pred,B,2,h,w), outs (n_pred,B,2,4h,4w); the mask is read and
 * soft-maxed once (models/MAGNET.py:173 upsamples every iteration's prediction with the same mask). */
MAGNET_API int magnet_upsample_depth_cl_n(const float *depths, const float *mask_pad, int32_t ld, float *outs, int32_t n_pred,
                                          int32_t B, int32_t h, int32_t w, void *stream);

/* Depth-error reductions on the device (utils.compute_depth_errors, utils/utils.py:106-144, with the masking /
 * clamping of test_MaGNet.py:43,58-79): pred (B,2,H*W) [mu, sigma], gt (B,H*W).  sums: OUT double (B,16), every
 * element written by the call (no memset needed): n, sum|d|, sum|d|/gt, sum d^2/gt, sum d^2, sum(ln gt-ln p)^2, sum(ln p-ln gt), sum|log10 gt-log10 p|,
 * sum(1/gt-1/p)^2, #(t<1.25), #(t<1.25^2), #(t<1.25^3), sum nll, 0,0,0.  The 12 metrics are ratios of these
 * (magnet_amd/metrics.py). */
MAGNET_API int magnet_depth_metrics(const float *pred, const float *gt, double *sums, int32_t B, int32_t HW,
                                    float min_depth, float max_depth, void *stream);
/* The same over the evaluation window rows [y0,y1) x columns [x0,x1) only: the reference's garg / eigen crops for KITTI
 * (test_MaGNet.py:63-71).  Both entry points sum in a fixed order (64 workgroups per frame
 * writing partial sums to a stream-ordered scratch allocation, then one fixed-order final sum): deterministic, no atomics. */
MAGNET_API int magnet_depth_metrics_crop(const float *pred, const float *gt, double *sums, int32_t B, int32_t H, int32_t W,
                                         float min_depth, float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1,
                                         void *stream);

/* The evaluation loops' form of the same reductions (additive to v400): the two planes are addressed through strides, the second
 * plane may hold the variance itself (test_DNet.py hands utils.compute_depth_errors the variance) or be absent (train_FNet.py's
 * validate() has no uncertainty), the partial sums go to a caller-provided work buffer (no allocation), and the second stage can
 * also write each frame's 12 metrics, so that an evaluation loop never reads anything back per batch. */
enum {                                     /* MagnetDepthMetricsArgs.kind: what the `second` planes hold */
    MAGNET_METRICS_SIGMA    = 0,           /* sigma: squared, then clamped at 1e-6; sums equal magnet_depth_metrics[_crop] to the bit */
    MAGNET_METRICS_VARIANCE = 1,           /* the variance, clamped at 1e-6 (utils.py:133-134) */
    MAGNET_METRICS_NONE     = 2            /* no second plane: sum 12 is 0 and the nll entry of every row is 0.0 */
};
typedef struct MagnetDepthMetricsArgs {
    const float *mu;                       /* B planes of H x W (rows contiguous), mu_stride elements apart */
    const float *second;                   /* sigma or variance planes, second_stride elements apart; NULL exactly when kind == NONE */
    const float *gt;                       /* (B, H, W) contiguous */
    int64_t      mu_stride, second_stride;
    int32_t      B, H, W, kind;
    float        min_depth, max_depth;
    int32_t      crop, y0, y1, x0, x1;     /* crop != 0: evaluate inside rows [y0, y1) x columns [x0, x1) */
    double      *sums;                     /* optional OUT (B, 16), as magnet_depth_metrics writes them */
    double      *rows;                     /* optional OUT (B, 12): per-frame abs_rel abs_diff sq_rel rmse rmse_log irmse log_10 silog a1 a2 a3
                                              nll, the fp64 expressions of magnet_amd/metrics.py's metrics_from_sums, each operation rounded
                                              on its own; a frame without a valid pixel gives NaN (nll 0.0 under NONE) */
    void        *work;                     /* magnet_depth_metrics_workspace(B) bytes of scratch */
} MagnetDepthMetricsArgs;
/* Bytes of `work` for B frames (B x 64 x 13 doubles); -(MAGNET_E_DIM) for B <= 0. */
MAGNET_API int64_t magnet_depth_metrics_workspace(int32_t B);
/* Two launches on `stream`, no allocation, no synchronisation; at least one of sums / rows must be given (8-byte aligned, as work). */
MAGNET_API int magnet_depth_metrics_ex(const MagnetDepthMetricsArgs *args, void *stream);

/* ---- training step of g_net / mask_head (train_MaGNet.py:87-98): loss, convex-upsampling backward, head backward, weight
 * gradients.  Additive to v400: new entry points with their own argument structs (zero-initialise, then fill).  Every sum is
 * taken in a fixed order with no atomics: results are bit-identical from run to run. */

#define MAGNET_NLL_BLOCKS   256            /* workgroups of the loss's first reduction stage */
#define MAGNET_NLL_MAX_ITER 16             /* n_iter limit of the loss */
#define MAGNET_WGRAD_CHUNK  2048           /* rows per partial tile of magnet_wgrad */

/* MagnetLoss, loss_fn 'gaussian' (utils/losses.py:28-52): for every iteration i, var = sigma^2 clamped to 1e-10 (no gradient
 * where the clamp applies), nll = (mu - gt)^2 / (2 var) + 0.5 log var averaged over the masked pixels, weighted by
 * gamma^(n_iter - 1 - i). */
typedef struct MagnetNllArgs {
    const float   *preds;                  /* (n_iter, B, 2, H, W) fp32 [mu, sigma] */
    const float   *gt;                     /* (B, H, W) */
    const uint8_t *mask;                   /* (B, H, W), 0 / 1 */
    double        *sums;                   /* (1 + n_iter): masked count, per-iteration NLL sums (forward writes, backward reads) */
    float         *loss;                   /* forward: the 0-d loss */
    double        *work;                   /* forward: MAGNET_NLL_BLOCKS * (1 + n_iter) doubles of scratch */
    const float   *grad_loss;              /* backward: device scalar dL/dloss (read on the device) */
    float         *grad_preds;             /* backward: (n_iter, B, 2, H, W), every element written */
    double         gamma;
    int32_t        n_iter, B, H, W;
} MagnetNllArgs;
MAGNET_API int magnet_nll_loss_forward(const MagnetNllArgs *args, void *stream);
MAGNET_API int magnet_nll_loss_backward(const MagnetNllArgs *args, void *stream);

/* Backward of the learned convex upsampling (models/MAGNET.py:15-27) for n_pred predictions sharing one mask:
 * grad_up (n_pred, B, 2, k h, k w), depth (n_pred, B, 2, h, w) -> grad_depth (same shape as depth) and grad_mask = the mask's
 * gradient summed over the predictions.  The mask's logit (b, ch, y, x), ch < 9 k k, sits at mask[b*mask_sb + ch*mask_sc +
 * y*mask_sy + x*mask_sx]; grad_mask's at grad_mask[b*gm_sb + ch*gm_sc + y*gm_sy + x*gm_sx] (only those elements are written).
 * work: n_pred*B*2*9*h*w floats. */
typedef struct MagnetUpsampleBwdArgs {
    const float *grad_up, *depth, *mask;
    float       *grad_depth, *grad_mask, *work;
    int64_t      mask_sb, mask_sc, mask_sy, mask_sx;
    int64_t      gm_sb, gm_sc, gm_sy, gm_sx;
    int32_t      n_pred, B, h, w, k;       /* k <= 8 */
} MagnetUpsampleBwdArgs;
MAGNET_API int magnet_upsample_depth_backward(const MagnetUpsampleBwdArgs *args, void *stream);

/* Backward through the 1x1 tail of a stack (models/MAGNET.py:53-55, :113-115): dh3 = W4^T dout [h3 > 0], dh2 = W3^T dh3 [h2 > 0],
 * dh1 = W2^T dh2 [h1 > 0] on the matrix cores (bf16x3).  Rows are the zero-bordered grid of magnet_conv_mfma (rows = B (h+2) (w+2));
 * every output is written on every row, zeros on the border rows.  G-Net form (dout == NULL, k0 = 32): dout = the Gaussian update's
 * backward (models/MAGNET.py:60-69) from grad_gmm, the head's fp32 output gnet_out (channel 1 = pre-ELU sigma) and gmm_in. */
typedef struct MagnetHeadDgradArgs {
    const float *dout;                     /* fp32 (rows, k0) gradient of the last layer's output, or NULL (G-Net form) */
    int32_t      k0;                       /* 32, 128 or 160: last layer's output channels padded to 32 */
    const void  *wt_hi, *wt_lo;            /* bf16 [W4^T (128, k0) | W3^T (128, 128) | W2^T (128, 128)] (nn.Conv2d weight transposed) */
    const void  *h3_hi, *h2_hi, *h1_hi;    /* bf16 hi planes (rows, 128) of the forward's post-ReLU activations */
    void        *dout_hi, *dout_lo;        /* out: split bf16 (rows, k0) of dout (input of the last layer's weight gradient) */
    void        *dh3_hi, *dh3_lo, *dh2_hi, *dh2_lo, *dh1_hi, *dh1_lo;   /* out: split bf16 (rows, 128) */
    float       *acc;                      /* optional fp32 (rows, 128): acc_mode 1 acc = dh1, 2 acc += dh1 */
    void        *acc_hi, *acc_lo;          /* optional: split bf16 of the updated acc */
    int32_t      acc_mode;
    int32_t      B, h, w;
    int64_t      rows;
    const float *grad_gmm;                 /* G-Net form: (B, 2, h, w) d(mu, sigma) of the update's output */
    const float *gnet_out;                 /* G-Net form: fp32 (rows, gnet_ld) */
    const float *gmm_in;                   /* G-Net form: (B, 2, h, w) the update's input (mu0, sigma0) */
    int32_t      gnet_ld;
} MagnetHeadDgradArgs;
MAGNET_API int magnet_head_dgrad(const MagnetHeadDgradArgs *args, void *stream);

/* Weight gradient of one convolution layer on the matrix cores (bf16x3, fp32 accumulation): dW[tap][o][c] = sum over the interior
 * rows [wp+1, rows-wp-1) of dy[row][o] * x[row + off(tap)][c], off = (tap/3 - 1) wp + (tap%3 - 1) for taps = 9; bias gradient
 * sum dy[row][o].  dy and x are split bf16 planes of the zero-bordered grid (dy zero on its border rows); x may be a channel
 * slice of a wider buffer (x_ld).  The result for o < cout_valid, c < cin_valid lands in grad_w laid out as nn.Conv2d's
 * (Cout, cin_total, kh, kw) at input channel cin_dst + c (accumulate = 1: added to what is there). */
typedef struct MagnetWgradArgs {
    const void *dy_hi, *dy_lo;
    const void *x_hi, *x_lo;
    int64_t     dy_ld, x_ld;               /* row pitches in elements (multiples of 8) */
    int64_t     rows;
    int32_t     cout, cin;                 /* channels read: multiples of 8 */
    int32_t     taps, wp;                  /* taps 1 or 9; wp = w + 2 */
    float      *grad_w;
    float      *grad_b;                    /* optional (cout_valid) */
    int32_t     cout_valid, cin_valid, cin_total, cin_dst;
    int32_t     accumulate;
    float      *work;                      /* magnet_wgrad_workspace(args) bytes */
} MagnetWgradArgs;
MAGNET_API int64_t magnet_wgrad_workspace(const MagnetWgradArgs *args);
MAGNET_API int magnet_wgrad(const MagnetWgradArgs *args, void *stream);

/* ---- F-Net forward in training mode (train_FNet.py:69-119 with model.train()): BatchNorm2d with the statistics of the batch.
 * Additive to v400: new entry points with their own argument struct (zero-initialise, then fill).  The statistics are summed in a
 * fixed order in fp64 with no atomics: results, running statistics included, are bit-identical from run to run. */

#define MAGNET_BN_BLOCKS 256               /* workgroups of the statistics' first reduction stage */

/* firstconv.0 of the F-Net without BatchNorm and ReLU: (N, 3, H, W) fp32 image, wgt (32, 27) fp32 -> fp32 (N, H2+2, W2+2, 32)
 * channel-last grid, H2 = (H-1)/2 + 1; only the interior is written. */
MAGNET_API int magnet_fnet_stem_raw(const float *img, const float *wgt, float *out, int32_t N, int32_t H, int32_t W, void *stream);

/* One BatchNorm2d in training mode over a channel-last grid: N images of hp x wp rows whose interior, rows (n, pad + y, pad + x)
 * for y < hp - 2 pad, x < wp - 2 pad, holds the layer's C channels (pad = 0: no border).
 * magnet_bn_train_stats: mean and invstd = 1 / sqrt(biased variance + eps) over the N (hp - 2 pad)(wp - 2 pad) interior positions;
 *   running_mean / running_var (optional) become (1 - m) running + m stat with the unbiased variance, m = momentum, or
 *   1 / (num_batches_tracked + 1) when momentum < 0 (nn.BatchNorm2d(momentum=None)); num_batches_tracked (optional) += 1.
 * magnet_bn_train_apply: y = (x - mean) invstd gamma + beta (+ res, split bf16, same grid) (ReLU if relu), written over the
 *   whole grid as split bf16 planes (out_hi / out_lo, border rows zero; may be a channel slice: out_ld) or, with out_f32,
 *   over the interior in fp32. */
typedef struct MagnetBnTrainArgs {
    const float *x;                        /* pre-BN fp32 activations, x_ld elements per row (multiple of 4) */
    int64_t      x_ld;
    int32_t      N, hp, wp, pad, C;        /* C a multiple of 8, C <= min(x_ld, 2048) */
    double      *work;                     /* stats: MAGNET_BN_BLOCKS * C * 2 doubles of scratch */
    float       *mean, *invstd;            /* (C): written by stats, read by apply */
    float       *running_mean, *running_var;
    int64_t     *num_batches_tracked;
    double       eps, momentum;
    const float *gamma, *beta;             /* (C) the affine parameters */
    const void  *res_hi, *res_lo;          /* optional residual (split bf16), res_ld elements per row */
    int64_t      res_ld;
    int32_t      relu;
    void        *out_hi, *out_lo;          /* split bf16 output, out_ld elements per row (multiple of 8) */
    float       *out_f32;                  /* or fp32 output (then out_hi / out_lo are ignored) */
    int64_t      out_ld;
} MagnetBnTrainArgs;
MAGNET_API int magnet_bn_train_stats(const MagnetBnTrainArgs *args, void *stream);
MAGNET_API int magnet_bn_train_apply(const MagnetBnTrainArgs *args, void *stream);

/* ---- F-Net backward in training mode (csrc/train_fnet_bwd.hip).  Fixed-order sums, no atomics: bit-identical from run to run. */

/* magnet_wgrad with other tap windows: taps 9 with dilation dil (>= 1), taps 4 = the space-to-depth 2x2 window (row offsets -wp-1,
 * -wp, -1, 0; grad_w laid out as (Cout, cin_total, 2, 2)), or taps 1.  The rows summed are those whose every tap stays inside
 * [0, rows); dy must be zero on the border rows, as for magnet_wgrad. */
typedef struct MagnetWgradExArgs {
    MagnetWgradArgs base;
    int32_t         dil;
    int32_t         reserved;
} MagnetWgradExArgs;
MAGNET_API int64_t magnet_wgrad_ex_workspace(const MagnetWgradExArgs *args);
MAGNET_API int magnet_wgrad_ex(const MagnetWgradExArgs *args, void *stream);

/* BatchNorm2d backward in training mode over the grid of magnet_bn_train_*: x the saved pre-BN activations, g the gradient of the
 * layer's output (interior rows read).  relu: the output was ReLU'd; the mask is recomputed from x exactly as the apply did.
 * dgamma = sum g' xhat, dbeta = sum g' (fp64 two-stage sums); dx = gamma invstd (g' - sum g' / n - xhat sum g' xhat / n) written as
 * split bf16 over the whole grid (border rows zero). */
typedef struct MagnetBnBwdArgs {
    const float *x;
    int64_t      x_ld;
    int32_t      N, hp, wp, pad, C;
    int32_t      relu;
    const float *mean, *invstd, *gamma, *beta;
    const float *g;
    int64_t      g_ld;
    double      *work;                     /* MAGNET_BN_BLOCKS * C * 2 + 2 * C doubles of scratch */
    float       *dgamma, *dbeta;           /* (C) */
    void        *dx_hi, *dx_lo;
    int64_t      dx_ld;
} MagnetBnBwdArgs;
MAGNET_API int magnet_bn_train_backward(const MagnetBnBwdArgs *args, void *stream);

/* (N, C, h, w) fp32 -> split bf16 planes of the zero-bordered grid (N, h+2pad, w+2pad, ld), channels [C, ld) and the border zero. */
MAGNET_API int magnet_fnet_grad_pack(const float *nchw, void *out_hi, void *out_lo, int32_t N, int32_t C, int32_t h, int32_t w,
                                     int32_t pad, int32_t ld, void *stream);
/* Backward of magnet_space_to_depth: in fp32 (N, H4+2ipad, W4+2ipad, 4C) -> out fp32 interior of (N, H2+2, W2+2, C). */
MAGNET_API int magnet_fnet_d2s_backward(const float *in, float *out, int32_t N, int32_t C, int32_t H2, int32_t W2, int32_t ipad,
                                        void *stream);

/* SPP backward.  magnet_spp_upsample_backward: gradient of the align_corners bilinear upsampling (ph x pw -> h x w), gathered per
 * pooled cell in a fixed order: g (interior of the (N, h+2pad, w+2pad, g_ld) fp32 grid, channels [c_off, c_off + 32)) -> dq
 * (N*ph*pw, 32).  magnet_spp_pool_backward: out (interior, 128 channels, out_ld) = g channels [c_off, c_off + 128) + sum over the
 * four branches (k = 64, 32, 16, 8) of dpool[b][cell] / k^2 where the floor pooling covers the position. */
typedef struct MagnetSppBwdArgs {
    const float *g;
    int64_t      g_ld;
    int32_t      N, h, w, pad, c_off;
    int32_t      ph, pw;
    float       *dq;
    const float *dpool[4];                 /* (N * (h/k) * (w/k), 128) for k = 64, 32, 16, 8 */
    float       *out;
    int64_t      out_ld;
} MagnetSppBwdArgs;
MAGNET_API int magnet_spp_upsample_backward(const MagnetSppBwdArgs *args, void *stream);
MAGNET_API int magnet_spp_pool_backward(const MagnetSppBwdArgs *args, void *stream);

/* Weight gradient of firstconv.0 (3 -> 32, 3x3 stride 2) from the NCHW fp32 image and dz (split bf16, (N, H2+2, W2+2, 32)):
 * grad_w (32, 3, 3, 3).  work: MAGNET_BN_BLOCKS * 864 doubles. */
MAGNET_API int magnet_fnet_stem_wgrad(const float *img, const void *dz_hi, const void *dz_lo, float *grad_w, double *work, int32_t N,
                                      int32_t H, int32_t W, void *stream);

/* ---- the D-Net decoder (DenseDepth_BN at downsample ratio 4, models/submodules/D_dense_depth.py:104-195; magnet_amd/dnet.py) ----
 * Its convolutions run on magnet_conv_mfma's kernel with BatchNorm folded into weights and bias; the bilinear upsampling and the skip
 * concatenation on magnet_upsample_bilinear_cl / magnet_pack_split. */

enum {                                     /* MagnetConvExArgs.act */
    MAGNET_ACT_BASE       = 0,             /* as magnet_conv_mfma: base.relu decides */
    MAGNET_ACT_LEAKY_RELU = 1,             /* LeakyReLU(act_slope) after bias / addend / residual (UpSampleBN._net, D_dense_depth.py:29-43):
                                              x < 0 -> x * act_slope.  Needs base.relu == 0 and no fused tail; every other output form
                                              (bf16 planes, fp32, single bf16 plane, channel slices, zero border, repad) applies it */
    MAGNET_ACT_SILU       = 2              /* SiLU after bias / addend / residual (the EfficientNet encoder's expand layers): x * sigmoid(x)
                                              = x / (1 + e), e = 2^(-x log2 e) on the hardware exponential (1 ulp), one fp32 add, one
                                              correctly rounded divide: |got - silu(x)| <= 2^-21 |silu(x)| + 2^-22.  Needs base.relu == 0
                                              and no fused tail; every output form MAGNET_ACT_LEAKY_RELU serves applies it.  Served by
                                              magnet_conv_mfma_ex only: the fp16 entry points and the split-K forms refuse it (MAGNET_E_DIM) */
};

enum {                                     /* MagnetConvExArgs.tiling: bit flags, for tests and A/B runs; 0 = the library chooses */
    MAGNET_TILING_FLAT  = 1,               /* cut the flattened rows into tiles from row 0 on, also where per-image tiling (launches with
                                              base.gu_in / base.up_depth) would take fewer workgroups.  Same kernel, same interior results. */
    MAGNET_TILING_BM256 = 2,               /* fused-tail 3x3 launches: the 256-row 8-wave kernel also below 65 536 rows */
    MAGNET_TILING_BM64  = 4                /* 64-row tiles of the 4-wave register-window kernel (latency mode: twice the workgroups of the
                                              128-row form, bit-identical results): 3x3 launches (taps == 9) with cout_pad == 128 and a
                                              fused tail, or plain with cout_pad % 128 == 0; not with BM256.
                                              Any other launch is refused with MAGNET_E_DIM */
};

/* magnet_conv_mfma with an activation mode.  act = MAGNET_ACT_BASE and the other fields zero give exactly magnet_conv_mfma(&args->base). */
typedef struct MagnetConvExArgs {
    MagnetConvArgs base;
    int32_t        act;                    /* MAGNET_ACT_* */
    float          act_slope;              /* negative slope of MAGNET_ACT_LEAKY_RELU (nn.LeakyReLU(): 0.01); finite */
    int32_t        tiling;                 /* MAGNET_TILING_* flags */
    int64_t       *tiles_out;              /* optional HOST pointer: receives the number of row tiles (workgroups along x) launched */
} MagnetConvExArgs;
MAGNET_API int magnet_conv_mfma_ex(const MagnetConvExArgs *args, void *stream);

/* The fused 3x3 launches of the inference step with part of their input read in place from an NCHW fp32 tensor: input channels
 * [src_c0, cin) are taken from `src` and split to (hi, lo) bf16 inside the kernel (hi = bf16(x), lo = bf16(x - hi), round to nearest
 * even: what magnet_pack_split writes), so no packed copy of them exists; channels [0, src_c0) come from ex.base.in_hi / in_lo as in
 * magnet_conv_mfma_ex (row pitch in_ld; the planes' channels from src_c0 on are never read, and in_hi / in_lo may be NULL when
 * src_c0 == 0).  The result is, bit for bit, that of magnet_conv_mfma_ex on planes that hold magnet_pack_split(src) in those channels.
 * Serves exactly: bf16x3 operands, taps == 9 without dilation, cout_pad == 128, the fused tail of 16 outputs with gu_in / gu_out or of
 * 144 outputs with up_depth / up_out, the 256-row kernel (rows >= 65 536 or MAGNET_TILING_BM256), no addend, act == MAGNET_ACT_BASE,
 * and per-image row tiling in effect (magnet_conv_row_tiles(up_B, up_h, wp, 256) reports tiles per image > 0; MAGNET_TILING_FLAT is
 * refused).  Everything else — MAGNET_TILING_BM64, the fp16 formats, a residual, border or repad form among it — is refused
 * with MAGNET_E_DIM, a NULL src with MAGNET_E_NULL, a misaligned one with MAGNET_E_ALIGN, before any launch.  tiles_out works. */
typedef struct MagnetConvNchwArgs {
    MagnetConvExArgs ex;
    const float   *src;                    /* (up_B, src_C, up_h, up_w) fp32, contiguous, 16-byte-aligned base */
    int32_t        src_c0;                 /* first input channel taken from src: multiple of 32, src_c0 + src_C == base.cin */
    int32_t        src_C;                  /* multiple of 32 */
} MagnetConvNchwArgs;
MAGNET_API int magnet_conv_mfma_nchw(const MagnetConvNchwArgs *args, void *stream);

/* The 3x3 layer of a G-Net / mask-head stack on the single-plane fp16 operand format (see MagnetConvArgs): base.in_hi / base.w_hi are
 * the fp16 planes; base.in_lo, base.w_lo must be NULL (MAGNET_E_DIM otherwise: planes of another format are
 * refused, not mis-read).  Serves what the inference loop launches and refuses the rest with MAGNET_E_DIM: taps == 9 without dilation,
 * cout_pad == 128, and either the fused tail with tail_cout_pad 16 or 144 (tail_w_hi / tail_w_lo bf16 planes; with gu_in / gu_out,
 * up_depth / up_out and addend as in magnet_conv_mfma) or the plain layer with fp32 output (out_mode 1, optional addend).  No residual,
 * border, repad, other out_mode, MAGNET_ACT_LEAKY_RELU or MAGNET_TILING_BM64; MAGNET_TILING_FLAT, MAGNET_TILING_BM256 and tiles_out work
 * as in magnet_conv_mfma_ex (256-row tiles from 65 536 rows on, for launches without an addend; else 128-row tiles). */
MAGNET_API int magnet_conv_mfma_f16(const MagnetConvExArgs *args, void *stream);

/* The single-plane fp16 format, plane to plane: the launches of an F-Net whose every activation buffer is ONE zero-bordered
 * channel-last fp16 plane (FNetMFMA(precision="fp16")).  The struct's fields mean, for this entry point only:
 *   base.in_hi / base.w_hi   fp16 planes (rows, in_ld) / (taps, cout_pad, cin); base.in_lo, w_lo and add_lo must be NULL
 *   base.add_hi              optional residual input, ONE fp16 plane with row pitch add_ld, added before bias / ReLU
 *   base.out_mode            3: one fp16 plane at out_hi (saturating round-to-nearest-even, NaN written through: see MagnetConvArgs);
 *                            1 (fp32 at out_f32) and 2 (one bf16 plane at out_hi) as in magnet_conv_mfma; 0 is refused
 *   border_hp / border_pad / repad / dil / in_ld / out_ld   as in magnet_conv_mfma
 * Serves taps 1, 4 and 9, cout_pad 32, 64 and 128, cin a multiple of 32, act == MAGNET_ACT_BASE, tiling 0 or MAGNET_TILING_FLAT (always
 * 128-row tiles); tiles_out works.  A fused tail, an addend, the Gaussian update / upsampling and MAGNET_TILING_BM64 /
 * MAGNET_TILING_BM256 are refused with MAGNET_E_DIM.  Each fp16 x fp16 product is exact in the fp32 accumulator; bias, residual and ReLU
 * are fp32 arithmetic as in magnet_conv_mfma. */
MAGNET_API int magnet_conv_mfma_f16p(const MagnetConvExArgs *args, void *stream);

/* Split-K form of the plain bf16x3 layer, for launches with too few row tiles to fill the chip (the D-Net decoder at one to a few
 * images): split s of split_k runs the K loop over the input-channel chunks [floor(s C / split_k), floor((s + 1) C / split_k)) of the
 * C = cin / 32 chunks, all taps, and stores its raw fp32 accumulators to work[s][row][cout_pad] (rows < base.rows); a second launch on
 * the same stream forms x = (((p_0 + p_1) + p_2) + ...) + bias in fp32, in ascending s, and applies magnet_conv_mfma_ex's epilogue:
 * ReLU / MAGNET_ACT_LEAKY_RELU, zeros at border positions, repad, out_ld channel slices, out_mode 0 (split-bf16 planes) or 1 (fp32).
 * No counters or atomics; deterministic.  A partial equals, to the bit, what magnet_conv_mfma writes to out_f32 for that channel range
 * alone (channel-offset input view, weights packed for the range, zero bias, no activation), so the result differs from the unsplit
 * launch by the order of split_k - 1 fp32 additions only.
 * Serves: 2 <= split_k <= MAGNET_SPLITK_MAX; taps 1 or 9 (dil as in magnet_conv_mfma); cout_pad a multiple of 128; every split at least
 * MAGNET_SPLITK_MIN_CHUNKS chunks ((cin / 32) / split_k >= MAGNET_SPLITK_MIN_CHUNKS; the K loop's ring itself runs from one chunk on —
 * two keep its prefetch in use); out_mode 0 or 1; tiling 0 or MAGNET_TILING_FLAT (128-row tiles); tiles_out works.  A fused tail,
 * addend, residual input, the Gaussian update / upsampling, MAGNET_TILING_BM64 / BM256 and any other out_mode are
 * refused with MAGNET_E_DIM; `work` NULL: MAGNET_E_NULL, not 16-byte aligned: MAGNET_E_ALIGN, work_bytes too small: MAGNET_E_DIM.  A
 * refused call writes nothing.  The workspace query returns split_k * rows * cout_pad * 4, or -(MAGNET_E_*) for a form that is refused. */
#define MAGNET_SPLITK_MAX        8
#define MAGNET_SPLITK_MIN_CHUNKS 2
MAGNET_API int64_t magnet_conv_mfma_splitk_workspace(const MagnetConvExArgs *args, int32_t split_k);
MAGNET_API int magnet_conv_mfma_splitk(const MagnetConvExArgs *args, int32_t split_k, float *work, int64_t work_bytes, void *stream);

/* The single-plane fp16 format, plane to plane and WIDE: the plain layers of a D-Net decoder whose activation buffers are ONE
 * zero-bordered channel-last fp16 plane each (DNetMFMA(precision="fp16")).  The struct's fields mean, for this entry point only:
 *   base.in_hi / base.w_hi   fp16 planes (rows, in_ld) / (taps, cout_pad, cin); base.in_lo, w_lo, add_hi and add_lo must
 *                            be NULL (planes of another format are refused, not mis-read; there is no residual input)
 *   act                      MAGNET_ACT_BASE (base.relu 0 or 1) or MAGNET_ACT_LEAKY_RELU(act_slope), as in magnet_conv_mfma_ex
 *   base.out_mode            3: one fp16 plane at out_hi (saturating round-to-nearest-even, NaN written through: see MagnetConvArgs);
 *                            1: fp32 at out_f32; 0: split-bf16 planes at out_hi / out_lo (x_feat for G-Net's buffer and the heads); 2 is
 *                            refused
 *   border_hp / border_pad / repad / in_ld / out_ld   as in magnet_conv_mfma
 * Serves taps 1 and 9 without dilation, cout_pad a multiple of 128 (128-row x 128-channel tiles, one grid column per 128 channels), cin
 * a multiple of 32, tiling 0 or MAGNET_TILING_FLAT; tiles_out works.  A fused tail, an addend, a residual input, the Gaussian update /
 * upsampling, dilation, any other cout_pad and MAGNET_TILING_BM64 / MAGNET_TILING_BM256 are refused with MAGNET_E_DIM;
 * a refused call writes nothing.  Each fp16 x fp16 product is exact in the fp32 accumulator; bias and activation are fp32 arithmetic
 * as in magnet_conv_mfma.  Domain: |activation|, |weight| <= 65504 (stores clamp; the caller rounds its weights). */
MAGNET_API int magnet_conv_mfma_f16d(const MagnetConvExArgs *args, void *stream);

/* Split-K form of magnet_conv_mfma_f16d: the contract of magnet_conv_mfma_splitk (chunk ranges, work[s][row][cout_pad] raw fp32
 * partials, the second launch summing in ascending s, then bias and the epilogue; limits, refusals, error codes and workspace query the
 * same; no counters or atomics) on the fp16 operand planes of magnet_conv_mfma_f16d, whose own refusals apply too.  The reduce also
 * serves out_mode 3 (one fp16 plane).  A partial equals, to the bit, what magnet_conv_mfma_f16d writes to out_f32 for that channel range
 * alone (channel-offset input view, weights packed for the range, zero bias, no activation). */
MAGNET_API int64_t magnet_conv_mfma_f16d_splitk_workspace(const MagnetConvExArgs *args, int32_t split_k);
MAGNET_API int magnet_conv_mfma_f16d_splitk(const MagnetConvExArgs *args, int32_t split_k, float *work, int64_t work_bytes, void *stream);

/* The single-plane fp16 format, plane to plane, for the 1x1 layers of the EfficientNet encoder (EncoderMFMA(precision="fp16")): what
 * magnet_conv_mfma_f16p refuses (SiLU) and what magnet_conv_mfma_f16d refuses (SiLU, a residual input), on the kernel instances of those
 * two — it adds no kernel.  The struct's fields mean, for this entry point only:
 *   base.in_hi / base.w_hi   fp16 planes (rows, in_ld) / (1, cout_pad, cin); base.in_lo, w_lo and add_lo must be NULL
 *   base.add_hi              optional residual input: ONE fp16 plane (rows, add_ld), added before the bias
 *   act                      MAGNET_ACT_BASE with base.relu == 0 (a linear layer), or MAGNET_ACT_SILU
 *   base.out_mode            3: one fp16 plane at out_hi (saturating round-to-nearest-even, NaN written through); 1: fp32 at out_f32
 *   border_hp / border_pad / repad / in_ld / out_ld   as in magnet_conv_mfma
 * Serves taps == 1, cout_pad 32, 64 or a multiple of 128, cin a multiple of 32, tiling 0 or MAGNET_TILING_FLAT; tiles_out works.  A fused
 * tail, an addend, the Gaussian update / upsampling, MAGNET_TILING_BM64 / MAGNET_TILING_BM256, every other value of taps, act and
 * out_mode, any other cout_pad (144 included: issue such a layer as launches on channel slices, out_ld) and relu == 1 are refused with
 * MAGNET_E_DIM before any launch; a refused call writes nothing.  With MAGNET_ACT_BASE the result equals, to the bit, what
 * magnet_conv_mfma_f16p (cout_pad 32 / 64) or magnet_conv_mfma_f16d (cout_pad % 128 == 0, no residual) writes.  Domain: |activation|,
 * |weight| <= 65504 (stores clamp; the caller rounds its weights). */
MAGNET_API int magnet_conv_mfma_f16e(const MagnetConvExArgs *args, void *stream);

/* fp32 NCHW (N, C, h, w) (image stride `in_img_stride` elements, 0 = C*h*w) -> channels [c_off, c_off + round_up(C, 8)) of the interior
 * of a zero-bordered (N, h+2, w+2, ctot) fp16 plane (the round-up lanes are written as zeros, as by magnet_pack_split).  ctot and c_off
 * multiples of 8.  The border rows and every other channel are not written.  Conversion: see the single-plane fp16 format above. */
MAGNET_API int magnet_pack_f16(const float *nchw, void *out_f16, int32_t N, int32_t C, int32_t h, int32_t w, int32_t ctot, int32_t c_off,
                               int64_t in_img_stride, void *stream);

/* Channels [c0, c1) of split-bf16 planes (rows, ld) -> the same channels of an fp16 plane (rows, ld16): f16(hi + lo), the sum formed in
 * fp32, converted as by magnet_pack_f16.  c0, c1, ld, ld16 multiples of 8; every row is converted (a zero border stays zero); nothing
 * outside [c0, c1) is written. */
MAGNET_API int magnet_planes_to_f16(const void *in_hi, const void *in_lo, int32_t ld, void *out_f16, int32_t ld16, int64_t rows,
                                    int32_t c0, int32_t c1, void *stream);

/* The F-Net's non-GEMM layers on the single-plane fp16 format: magnet_fnet_stem, magnet_space_to_depth, magnet_avgpool_cl and
 * magnet_upsample_bilinear_cl with ONE fp16 plane wherever those take a (hi, lo) pair.  Same geometry, same fp32 arithmetic; values
 * are stored as magnet_pack_f16 stores them (space_to_depth moves 2-byte values unchanged). */
MAGNET_API int magnet_fnet_stem_f16(const float *img, const float *wgt, const float *bias, void *out_f16, int32_t N, int32_t H, int32_t W,
                                    void *stream);
MAGNET_API int magnet_space_to_depth_f16(const void *in_f16, void *out_f16, int32_t N, int32_t C, int32_t H2, int32_t W2, int32_t opad,
                                         void *stream);
MAGNET_API int magnet_avgpool_cl_f16(const void *in_f16, int32_t ld, int32_t N, int32_t h, int32_t w, int32_t pad, int32_t k, int32_t C,
                                     void *out_f16, void *stream);
MAGNET_API int magnet_upsample_bilinear_cl_f16(const float *in, int32_t in_ld, int32_t ph, int32_t pw, int32_t C, void *out_f16,
                                               int32_t out_ld, int32_t N, int32_t h, int32_t w, int32_t pad, void *stream);

/* Row tiling of the launches that know their image geometry (base.gu_in / base.up_depth): the number of bm-row tiles (workgroups
 * along x) for n_img zero-bordered (h + 2, wp) grids, and in *tiles_per_img (optional) the tiles per image, or 0 for flat tiling.
 * Flat: tile t covers rows [t bm, (t + 1) bm) of the flattened buffer, ceil(n_img (h + 2) wp / bm) tiles.  Per image: tile t of image i
 * covers the bm rows from i (h + 2) wp + wp + t bm on, ceil(h wp / bm) tiles per image; the top and bottom border image rows get no
 * tile.  Per-image tiling is used only when it takes fewer tiles than flat and an image's last tile ends inside that image.  Host
 * arithmetic only (no GPU needed); returns 0 on bad dimensions.  bm is 256 for fused-tail 3x3 launches of at least 65 536 rows, else 128
 * (64 under MAGNET_TILING_BM64). */
MAGNET_API int64_t magnet_conv_row_tiles(int32_t n_img, int32_t h, int32_t wp, int32_t bm, int32_t *tiles_per_img);

/* The D-Net's Gaussian activation behind its depth head (activation_G_magnet, models/DNET.py:62-67): from the head's fp32 output
 * `in` (rows, in_ld) over zero-bordered (N, h+2*pad, w+2*pad) grids (channel 0 = mu, channel 1 = v; border rows are not read)
 * -> out (N, 2, h, w) fp32 = [mu, sqrt(elu(v) + 1 + 1e-10)].  in_ld even, `in` 8-byte aligned. */
MAGNET_API int magnet_dnet_gauss_head(const float *in, int32_t in_ld, int32_t N, int32_t h, int32_t w, int32_t pad, float *out,
                                      void *stream);

/* The stand-alone D-Net's tail (DNET(dnet=True): upsample_depth_via_mask, models/submodules/D_dense_depth.py:85-100,187-192, then
 * activation_G, models/DNET.py:55-60) in one launch.  `head`: the depth head's fp32 output (rows, head_ld) over (N, h+2, w+2) grids,
 * channel 0 = mu, channel 1 = v, as magnet_dnet_gauss_head reads it; `mask`: the mask head's logits (rows, mask_ld) over the same
 * grids, channel n*16 + i*4 + j, as magnet_upsample_depth_cl reads them.  out (N, 2, 4h, 4w) fp32 NCHW, every element written:
 *   w[n] = softmax over the 9 taps n of mask[.., n*16 + i*4 + j]
 *   up[c][4y+i][4x+j] = sum_n w[n] * head[c] at (y + n/3 - 1, x + n%3 - 1), zero outside the image (F.unfold(padding=1); decided
 *                       by index: border rows of `head` are not read)
 *   out = [up[0], elu(up[1]) + 1 + 1e-10]      -- the RAW (mu, v) are upsampled, the activation follows at full resolution.
 * k = 4 only.  head_ld even and >= 2, `head` 8-byte aligned; mask_ld >= 144 and a multiple of 4, `mask` and `out` 16-byte aligned. */
MAGNET_API int magnet_dnet_upsample_gauss(const float *head, int32_t head_ld, const float *mask, int32_t mask_ld, int32_t N,
                                          int32_t h, int32_t w, float *out, void *stream);

/* ---- the D-Net's encoder (EfficientNet-B5, models/submodules/D_dense_depth.py:7-25; magnet_amd/encoder.py) ----
 * Its 1x1 layers run on magnet_conv_mfma_ex (MAGNET_ACT_SILU for the expand layers, add_hi / add_lo for the skip connection); the stem,
 * the depthwise convolutions and squeeze-excite are the entry points below.  Activations are the convolution kernel's format
 * throughout: zero-bordered channel-last grids (N, h+2, w+2, C_pad) as split-bf16 planes (hi, lo), C_pad a multiple of 32, pad
 * channels zero in both planes, border rows zero.  sigmoid and SiLU are MAGNET_ACT_SILU's forms (|sigmoid error| <= 2^-21).  Every
 * entry point checks its arguments on the host before any launch; a refused call writes nothing.  No atomics: results are deterministic. */

/* The stem: NCHW fp32 image (N, 3, H, W) -> the interior of planes (N, H2+2, W2+2, 64), H2 = ceil(H / 2), W2 = ceil(W / 2):
 * silu(bias[co] + sum W[co][ci][dy][dx] img[ci][2y + dy - pt][2x + dx - pl]), 3x3 stride 2 with TF "SAME" padding (total = max((H2 - 1) 2
 * + 3 - H, 0), pt = total / 2: 0 on an even H, 1 on an odd one; out-of-image taps decided by index).  wgt (48, 27) fp32 with BatchNorm
 * folded, bias (48); fp32 fmaf in the order ci, dy, dx.  Channels 48..63 are written zero; border rows are not written. */
MAGNET_API int magnet_enc_stem(const float *img, const float *wgt, const float *bias, void *out_hi, void *out_lo, int32_t N, int32_t H,
                               int32_t W, void *stream);

/* Depthwise k x k convolution + bias + SiLU, and the partial channel sums of its outputs for the squeeze.
 * out[n][oy][ox][c] = silu(bias[c] + sum_{ky,kx} wgt[ky k + kx][c] in[n][oy stride + ky - pad_top][ox stride + kx - pad_left][c]) for
 * oy < ho = ceil(h / stride), ox < wo = ceil(w / stride); taps outside the (h, w) image are skipped by index (the input grid's border is
 * never read); fp32 fmaf in the order ky, kx.  The interior of the output grid (N, ho+2, wo+2, out_ld) is written, all c_pad channels
 * (wgt and bias are zero in the pad lanes, so these stay zero).  part (N, n_part, c_pad) fp32: row t of image n holds the sum of the
 * fp32 outputs (after SiLU, before the bf16 split) of output tile t (8 rows x 16 columns, row-major over the image) — each owned by one
 * workgroup and written exactly once, in a fixed order.  n_part must equal magnet_dwconv_cl_parts(ho, wo). */
typedef struct MagnetDwConvArgs {
    const void  *in_hi, *in_lo;            /* (N, h+2, w+2, in_ld) split-bf16 planes */
    const float *wgt;                      /* [k*k][c_pad] fp32 */
    const float *bias;                     /* [c_pad] */
    void        *out_hi, *out_lo;          /* (N, ho+2, wo+2, out_ld) split-bf16 planes */
    float       *part;                     /* (N, n_part, c_pad) */
    int32_t      N, h, w, c_pad;           /* c_pad % 32 == 0 */
    int32_t      in_ld, out_ld;            /* row pitches in elements: >= c_pad, multiples of 8 */
    int32_t      k, stride;                /* 3 or 5; 1 or 2 */
    int32_t      pad_top, pad_left;        /* 0 .. k - 1 */
    int32_t      n_part;
} MagnetDwConvArgs;
MAGNET_API int64_t magnet_dwconv_cl_parts(int32_t ho, int32_t wo);
MAGNET_API int magnet_dwconv_cl(const MagnetDwConvArgs *args, void *stream);

/* The squeeze-excite gate, one workgroup per image: mean[c] = (part[n][0][c] + part[n][1][c] + ... in ascending order) / hw;
 * r[j] = silu(b_reduce[j] + sum_c w_reduce[j][c] mean[c]); gate[n][c] = sigmoid(b_expand[c] + sum_j w_expand_t[j][c] r[j]) for c < C,
 * 0 for C <= c < c_pad.  Both matrices are (R, C) fp32 (the expand matrix transposed).  1 <= C <= c_pad <= 8192, 1 <= R <= 1024; part is
 * 16-byte aligned.  The reduce sum of one j is formed by 64 lanes (lane l: channel quads 4 (l + 64 i), i ascending) and a fixed tree. */
MAGNET_API int magnet_se_gate(const float *part, int32_t n_part, int64_t hw, const float *w_reduce, const float *b_reduce,
                              const float *w_expand_t, const float *b_expand, int32_t C, int32_t R, int32_t c_pad, float *gate, int32_t N,
                              void *stream);

/* out = split(float(hi + lo) * gate[n][c]) over the interior of a grid (N, h+2, w+2, .), channels [0, c_pad); out may be the input. */
MAGNET_API int magnet_se_scale(const void *in_hi, const void *in_lo, int32_t in_ld, const float *gate, int32_t N, int32_t h, int32_t w,
                               int32_t c_pad, void *out_hi, void *out_lo, int32_t out_ld, void *stream);

/* The same three layers on the single-plane fp16 format (EncoderMFMA(precision="fp16")): every grid is ONE zero-bordered channel-last
 * fp16 plane where the entry points above take a (hi, lo) pair.  Same geometry, tiling, fp32 arithmetic and order; a value is read
 * exactly (fp16 -> fp32) and stored as magnet_pack_f16 stores it (saturating round-to-nearest-even: the stored value is within 2^-11
 * of the fp32 value, relative, inside the domain |x| <= 65504).  The depthwise partial sums are taken from the fp32 values BEFORE the
 * store, so magnet_se_gate is used unchanged and the squeeze mean does not see the fp16 rounding.
 *   magnet_enc_stem_f16    out_f16 (N, H2+2, W2+2, 64)
 *   magnet_dwconv_cl_f16   MagnetDwConvArgs with in_hi / out_hi the fp16 planes; in_lo and out_lo must be NULL (MAGNET_E_DIM otherwise:
 *                          planes of the other format are refused, not mis-read)
 *   magnet_se_scale_f16    out = f16(float(in) * gate[n][c]); out may be the input
 * Refusals and error codes are those of the (hi, lo) forms, under these names. */
MAGNET_API int magnet_enc_stem_f16(const float *img, const float *wgt, const float *bias, void *out_f16, int32_t N, int32_t H, int32_t W,
                                   void *stream);
MAGNET_API int magnet_dwconv_cl_f16(const MagnetDwConvArgs *args, void *stream);
MAGNET_API int magnet_se_scale_f16(const void *in_f16, int32_t in_ld, const float *gate, int32_t N, int32_t h, int32_t w, int32_t c_pad,
                                   void *out_f16, int32_t out_ld, void *stream);

/* Sequence inference (magnet_amd/sequence.py): a frame pool of n_slots slots keeps one frame's backbone outputs per slot, in the
 * layouts the kernels read:
 *   pool_feat  (n_slots, h+2, w+2, F) channel-last F-Net features, zero border, fp32 or bf16 (feat_dtype), F % 8 == 0
 *   pool_gmm   (n_slots, 2, h, w) fp32 [mu, sigma]
 *   pool_xd3_hi / pool_xd3_lo (n_slots, (h+2)(w+2), 256) split-bf16 planes of x_d3, zero border rows
 * magnet_gather_views assembles the inputs of one refinement step of B windows with V source views in one launch.  `slots`
 * ((1 + V) B int32, on the device): entry [b] is the slot of window b's reference frame, entry [B + v B + b] the slot of its view v
 * (view-major, as nghbr_imgs and src_pad).  Destinations, each optional (NULL skips it; gin_hi and gin_lo go together):
 *   ref_cl  (B, h, w, F)          the interior of the reference slot's features
 *   src_pad (V B, h+2, w+2, F)    whole padded frames
 *   ref_gmm (B, 2, h, w), src_gmm (V B, 2, h, w)
 *   gin_hi / gin_lo               the reference slot's 256 x_d3 channels into channels [gin_c_off, gin_c_off + 256) of rows
 *                                 [b (h+2)(w+2), (b+1)(h+2)(w+2)) of planes of row pitch gin_ld elements (MAGNET.gnet_input_buffer);
 *                                 no other channel is written
 * An entry < 0 or >= n_slots means "no frame": its destination is filled with zeros and nothing is read for it; the kernel never
 * reads outside the pool whatever the table holds.  Values are copied bit for bit.
 * pool_feat, the x_d3 planes, ref_cl, src_pad, gin_hi and gin_lo 16-byte aligned, gin_ld % 8 == 0, gin_c_off % 8 == 0; the
 * (mu, sigma) tensors only 4-byte (16-byte vectors are used where a source and its destination frame allow).  A pool tensor may be
 * NULL when no destination reads it. */
typedef struct MagnetGatherViewsArgs {
    const int32_t *slots;                  /* ((1 + V) B) int32 on the device */
    int32_t        n_slots;
    int32_t        B, V, h, w, F;
    int32_t        feat_dtype;             /* MAGNET_FEAT_* */
    const void    *pool_feat;
    const float   *pool_gmm;
    const void    *pool_xd3_hi;
    const void    *pool_xd3_lo;
    void          *ref_cl;
    void          *src_pad;
    float         *ref_gmm;
    float         *src_gmm;
    void          *gin_hi;
    void          *gin_lo;
    int64_t        gin_ld;
    int32_t        gin_c_off;
} MagnetGatherViewsArgs;
MAGNET_API int magnet_gather_views(const MagnetGatherViewsArgs *args, void *stream);

/* magnet_scatter_frames is the inverse of magnet_gather_views: it writes the staged backbone outputs of n frames into the pool in one
 * launch.  `slots` (n int32, on the device): entry [j] is the destination slot of staged frame j, so the launch has the same
 * arguments whatever slots the host picked (a captured HIP graph replays it with another table).  Sources, each optional (NULL skips
 * it and leaves its pool tensor untouched; xd3_hi and xd3_lo go together); a source that is given needs its pool tensor:
 *   feat            (n, h+2, w+2, F) padded channel-last features in feat_dtype
 *   gmm             (n, 2, h, w) fp32 [mu, sigma]
 *   xd3_hi / xd3_lo (n, (h+2)(w+2), 256) split-bf16 planes
 * Whole frames are copied bit for bit, borders included.  An entry < 0 or >= n_slots means "skip this frame": nothing is written for
 * it.  Every destination offset is slot x frame + (offset inside one frame): the kernel never writes outside the pool whatever the
 * table holds.  Two entries that name the same slot are the caller's error: one of the two frames wins, per 32 KiB piece of the frame
 * (the slot may end up holding pieces of both).
 * feat, the x_d3 planes and their pool tensors 16-byte aligned, F % 8 == 0; gmm, pool_gmm and slots only 4-byte (16-byte vectors are
 * used where a source frame and its destination are misaligned alike, single floats otherwise). */
typedef struct MagnetScatterFramesArgs {
    const int32_t *slots;                  /* (n) int32 on the device: destination slot of staged frame j */
    int32_t        n_slots;
    int32_t        n, h, w, F;
    int32_t        feat_dtype;             /* MAGNET_FEAT_* */
    const void    *feat;
    const float   *gmm;
    const void    *xd3_hi;
    const void    *xd3_lo;
    void          *pool_feat;
    float         *pool_gmm;
    void          *pool_xd3_hi;
    void          *pool_xd3_lo;
} MagnetScatterFramesArgs;
MAGNET_API int magnet_scatter_frames(const MagnetScatterFramesArgs *args, void *stream);

/* magnet_image_prep_u8: N raw camera frames of one size, uint8 channel-last (N, Hin, Win, 3), to the (N, 3, Hout, Wout) fp32 NCHW
 * tensor the backbones read, in one launch (csrc/image_prep.hip; magnet_amd/ingest.py builds the tables):
 *   1. crop: the box (crop_left, crop_top, crop_w, crop_h) of every frame, the semantics of PIL's im.crop(box) for a box inside the
 *      frame.  No byte outside the box is read.
 *   2. resize to (Wout, Hout) as PIL's Image.resize(..., resample=BILINEAR) does on 8-bit images: horizontal pass, then vertical pass
 *      over its uint8 result, each   ss = (1 << 21) + sum_k coef[xx][k] * pixel[xmin[xx] + k];  out = clamp(ss >> 22, 0, 255)   in
 *      int32.  coef_* is (out size, k*) int32, bounds_* (out size, 2) int32 rows of (xmin, n) with n <= k* taps used, both relative
 *      to the crop box.  A pass whose output size equals its input size (crop_w == Wout, crop_h == Hout) is skipped, its tables are
 *      not read and may be NULL, its k* is ignored.  Otherwise k* must be 2 * ceil(max(in / out, 1)) + 1, PIL's row length, and at
 *      most MAGNET_IMAGE_PREP_KMAX: a larger downscale ratio returns MAGNET_E_SHAPE.
 *   3. normalise: out[n][c][y][x] = lut[c * 256 + v] for the 8-bit result v; lut is (3, 256) fp32, the caller's normalisation of
 *      every byte value per channel.  The kernel does no floating-point arithmetic.
 * src_pitch: bytes between rows (>= 3 * Win), src_frame: bytes between frames (>= Hin * src_pitch).  The tables and out 4-byte
 * aligned.  The tables are read from device memory unchecked by the host; the kernel clamps every window into the crop box and every
 * tap count to k*, so tables other than the ones above give other pixels, never an access outside src's crop box or out.
 * Limits: N <= 65535, every size <= 32768 (MAGNET_E_DIM). */
#define MAGNET_IMAGE_PREP_KMAX 17          /* taps per axis: downscale ratios up to 8 */
typedef struct MagnetImagePrepArgs {
    const uint8_t *src;                    /* (N, Hin, Win, 3) uint8 through src_frame / src_pitch */
    int64_t        src_pitch, src_frame;   /* bytes */
    const int32_t *coef_x;                 /* (Wout, kx) */
    const int32_t *bounds_x;               /* (Wout, 2) */
    const int32_t *coef_y;                 /* (Hout, ky) */
    const int32_t *bounds_y;               /* (Hout, 2) */
    const float   *lut;                    /* (3, 256) */
    float         *out;                    /* (N, 3, Hout, Wout) dense */
    int32_t        N, Hin, Win;
    int32_t        crop_left, crop_top, crop_w, crop_h;
    int32_t        Hout, Wout;
    int32_t        kx, ky;
} MagnetImagePrepArgs;
MAGNET_API int magnet_image_prep_u8(const MagnetImagePrepArgs *args, void *stream);

/* Training samples (csrc/image_prep.hip, csrc/depth_prep.hip; magnet_amd/ingest.py: TrainPrep).  Both entry points read one record per
 * frame from device memory,
 *     frame_params: int32 (N, 4) = (lut_index, flip, win_x, win_y),
 * and produce, of the Hres x Wres image R that the resize of the crop box gives (the crop box itself where the sizes are equal), the
 * window   O[y][x] = R[win_y + y][flip ? Wres - 1 - (win_x + x) : win_x + x],   0 <= y < Hout, 0 <= x < Wout:   a horizontal flip
 * first, then a crop window of the flipped image.  The records are not trusted: lut_index is clamped to [0, n_luts), flip is any
 * non-zero value, the window origin is clamped into [0, Wres - Wout] x [0, Hres - Hout]; with records that respect these ranges no
 * clamp acts.
 *
 * magnet_train_prep_u8: magnet_image_prep_u8's computation (the same crop, the same two integer passes from the same tables, which are
 * built for crop_w -> Wres and crop_h -> Hres and have Wres / Hres rows; the same limits and the same clamps on the tables) with
 *     out[n][c][y][x] = luts[lut_index[n]][c][O_c[y][x]],   luts (n_luts, 3, 256) fp32:
 * the augmentation of a sample (gamma, brightness, colour, clip) and the normalisation are functions of (byte value, channel) and
 * arrive as one table per augmented sample.  No floating-point arithmetic happens on the device.
 *
 * magnet_depth_prep_u16: uint16 depth maps (N, Hin, Win) through src_pitch / src_frame (in ELEMENTS), the crop box, and PIL's NEAREST
 * resize as index tables: idx_x (Wres) / idx_y (Hres) int32 hold the source column / row inside the crop box of every resized column /
 * row; each is NULL exactly when that axis is not resized (crop_w == Wres / crop_h == Hres).  Every index is clamped into the box.
 *     out[n][0][y][x] = (v == invalid_code ? 0 : (float)v) / divisor,   v = O[y][x],
 * one correctly rounded fp32 division (not a multiplication by a reciprocal).  invalid_code -1: none.  divisor finite and > 0.
 * frame_params' lut_index is ignored.  Limits as magnet_image_prep_u8's: N <= 65535, every size <= 32768; the tables, frame_params and
 * out 4-byte aligned, the uint16 source 2-byte aligned. */
typedef struct MagnetTrainPrepArgs {
    const uint8_t *src;                    /* (N, Hin, Win, 3) uint8 through src_frame / src_pitch */
    int64_t        src_pitch, src_frame;   /* bytes */
    const int32_t *coef_x;                 /* (Wres, kx) */
    const int32_t *bounds_x;               /* (Wres, 2) */
    const int32_t *coef_y;                 /* (Hres, ky) */
    const int32_t *bounds_y;               /* (Hres, 2) */
    const float   *luts;                   /* (n_luts, 3, 256) */
    const int32_t *frame_params;           /* (N, 4) */
    float         *out;                    /* (N, 3, Hout, Wout) dense */
    int32_t        N, Hin, Win;
    int32_t        crop_left, crop_top, crop_w, crop_h;
    int32_t        Hres, Wres;             /* the resized image the tables are built for */
    int32_t        Hout, Wout;             /* the window: Hout <= Hres, Wout <= Wres */
    int32_t        kx, ky;
    int32_t        n_luts;
} MagnetTrainPrepArgs;
MAGNET_API int magnet_train_prep_u8(const MagnetTrainPrepArgs *args, void *stream);

typedef struct MagnetDepthPrepArgs {
    const uint16_t *src;                   /* (N, Hin, Win) uint16 through src_frame / src_pitch */
    int64_t        src_pitch, src_frame;   /* elements */
    const int32_t *idx_x;                  /* (Wres), or NULL when crop_w == Wres */
    const int32_t *idx_y;                  /* (Hres), or NULL when crop_h == Hres */
    const int32_t *frame_params;           /* (N, 4) */
    float         *out;                    /* (N, 1, Hout, Wout) dense */
    int32_t        N, Hin, Win;
    int32_t        crop_left, crop_top, crop_w, crop_h;
    int32_t        Hres, Wres;
    int32_t        Hout, Wout;
    int32_t        invalid_code;           /* a sample equal to it becomes 0; -1: none */
    float          divisor;
} MagnetDepthPrepArgs;
MAGNET_API int magnet_depth_prep_u16(const MagnetDepthPrepArgs *args, void *stream);

/* FnetLoss: the tail of the F-Net training step (train_FNet.py:95-104) on the raw volume x (B, D, h, w) of
 * magnet_cost_volume_cw(mode = 1): p = softmax over the D bins, pred = sum_j p_j d_j, loss = mean over the valid pixels of
 * |pred - gt|, valid iff gt > min_depth && !(gt > max_depth) (the driver's gt[gt > max_depth] = 0; mask = gt > min_depth, which needs
 * min_depth >= 0).  1 <= D <= MAGNET_MAX_CANDIDATES.  Forward: one ascending pass over x (online softmax in fp32, accurate expf);
 * writes pred, and with gt != NULL also m (the per-pixel maximum), rz (1 / sum_j exp(x_j - m)), sums and loss (NaN when no pixel is
 * valid).  With gt == NULL only x, d and pred are used: the expected depth alone (validate(), train_FNet.py:166-167).
 * Backward: grad_x_j = grad_loss / count * sign(pred - gt) * p_j * (d_j - pred) on valid pixels (sign(0) = 0), 0 elsewhere; every
 * element of grad_x is written; grad_loss and count are read on the device.  The loss is summed in fp64 by MAGNET_NLL_BLOCKS
 * workgroups and then in a fixed order: no atomics, bit-identical from run to run. */
typedef struct MagnetFnetLossArgs {
    const float   *x;                      /* (B, D, h, w) fp32 contiguous: the raw (pre-softmax) volume */
    const float   *d;                      /* (D) fp32 bin centres, on the device */
    const float   *gt;                     /* (B, h, w) fp32 at the volume's resolution, or NULL (forward: pred only) */
    float         *pred;                   /* (B, h, w): forward writes, backward reads */
    float         *m;                      /* (B, h, w): forward writes (gt != NULL), backward reads */
    float         *rz;                     /* (B, h, w): forward writes (gt != NULL), backward reads */
    double        *sums;                   /* (2): valid count, sum of |pred - gt| (forward writes, backward reads) */
    float         *loss;                   /* forward: the 0-d loss */
    double        *work;                   /* forward: MAGNET_NLL_BLOCKS * 2 doubles of scratch */
    const float   *grad_loss;              /* backward: device scalar dL/dloss (read on the device) */
    float         *grad_x;                 /* backward: (B, D, h, w), every element written */
    float          min_depth, max_depth;
    int32_t        B, D, h, w;
} MagnetFnetLossArgs;
MAGNET_API int magnet_fnet_loss_forward(const MagnetFnetLossArgs *args, void *stream);
MAGNET_API int magnet_fnet_loss_backward(const MagnetFnetLossArgs *args, void *stream);

/* ---- Synchronised BatchNorm (nn.SyncBatchNorm: train_FNet.py:220-222 converts every BatchNorm and trains under DDP): the statistics
 * of magnet_bn_train_stats / magnet_bn_train_backward taken over the shards of several ranks.  The library runs the device arithmetic
 * before and after the collective; the caller all-gathers the fp64 buffer in between (one all-gather per BatchNorm and direction).
 * Additive to v400: the existing argument structs plus plain parameters.  All four take C a multiple of 8 up to 2048 and a rank with
 * at least ONE interior position (magnet_bn_train_apply accepts one position too; only magnet_bn_train_stats needs two).
 * Every sum runs in fp64 in a fixed order (positions, then ranks in rank order) with no atomics, and the merge reads the same gathered
 * bytes on every rank: mean, invstd, n_tot and the running statistics are bit-identical across ranks and from run to run.
 *
 * magnet_bn_sync_moments: over the grid of MagnetBnTrainArgs (x, x_ld, N, hp, wp, pad, C, work as for magnet_bn_train_stats; the
 *   other fields are ignored) writes the rank's record, record[(3, C)] = (n, mean, M2): n the local count, M2 = sum (x - mean)^2.
 *   Writes neither mean / invstd nor the running statistics.
 * magnet_bn_sync_merge: records (world, 3, C), the ranks' records in rank order.  n_tot = sum n_r, mean = sum n_r mean_r / n_tot,
 *   M2 = sum (M2_r + n_r (mean_r - mean)^2).  Writes args->mean, args->invstd = 1 / sqrt(M2 / n_tot + eps), n_tot[0] (a device
 *   double, read by the backward) and updates running_mean / running_var / num_batches_tracked as magnet_bn_train_stats does, with
 *   the global unbiased variance M2 / (n_tot - 1).  Uses C, mean, invstd, eps, momentum and the running buffers of args; n_tot >= 2
 *   is the caller's to ensure (two ranks with a position each do).  magnet_bn_train_apply then runs on the shard unchanged.
 * magnet_bn_sync_backward_sums: over MagnetBnBwdArgs (mean / invstd the GLOBAL ones; dx_* ignored) writes sums[(2, C)] = (sum g',
 *   sum g' xhat) of the rank, and dgamma / dbeta as these LOCAL sums (torch.nn.SyncBatchNorm does the same; DDP averages them).
 * magnet_bn_sync_backward_apply: sums (world, 2, C) in rank order, added in that order; dx = gamma invstd (g' - sum g' / n_tot -
 *   xhat sum g' xhat / n_tot) with the device-side n_tot, written as magnet_bn_train_backward writes it (dgamma / dbeta ignored).
 *   work: MAGNET_BN_BLOCKS * C * 2 + 2 * C doubles, as for magnet_bn_train_backward. */
MAGNET_API int magnet_bn_sync_moments(const MagnetBnTrainArgs *args, double *record, void *stream);
MAGNET_API int magnet_bn_sync_merge(const MagnetBnTrainArgs *args, const double *records, int32_t world, double *n_tot, void *stream);
MAGNET_API int magnet_bn_sync_backward_sums(const MagnetBnBwdArgs *args, double *sums, void *stream);
MAGNET_API int magnet_bn_sync_backward_apply(const MagnetBnBwdArgs *args, const double *sums, int32_t world, const double *n_tot,
                                             void *stream);

/* DnetLoss: the tail of the stand-alone D-Net's training step behind the two head convolutions (upsample_depth_via_mask,
 * models/submodules/D_dense_depth.py:86-100; activation_G, models/DNET.py:56-60; DnetLoss 'gaussian', utils/losses.py:8-24) in
 * fused kernels.  depth (B, 2, h, w) is the RAW head output [mu, v]; the mask logit (b, ch, y, x), ch = t*16 + i*4 + j < 144 with
 * t = 3 (dy + 1) + (dx + 1) (unfold order), sits at mask[b*mask_sb + ch*mask_sc + y*mask_sy + x*mask_sx] and its gradient at
 * grad_mask[b*gm_sb + ch*gm_sc + y*gm_sy + x*gm_sx] (element strides, as MagnetUpsampleBwdArgs).  Per fine pixel (4y+i, 4x+j):
 *   w_t = softmax over the 9 taps; mu = sum_t w_t depth[0](y+dy, x+dx), vu likewise for depth[1] (zero outside the image, by index);
 *   var = (elu(vu) + 1) + 1e-10; nll = (mu - gt)^2 / (2 var) + 0.5 log var; loss = mean of nll over the pixels with valid != 0.
 * The arithmetic of the upsampling is magnet_dnet_upsample_gauss's, operation for operation: pred is that entry point's output to
 * the bit.  Forward writes pred (optional), sums and loss (NaN when no pixel is valid).  Backward recomputes the softmax from the
 * logits and writes every element of grad_depth and all 144 channels of grad_mask at every pixel (zeros when no pixel is valid);
 * grad_loss and the count are read on the device.  Sums are taken in fp64 per workgroup and then in a fixed order: no atomics,
 * bit-identical from run to run.  k = 4 only.  gt and pred 16-byte aligned, valid 4-byte aligned. */
typedef struct MagnetDnetLossArgs {
    const float   *depth;                  /* (B, 2, h, w) fp32 contiguous: the raw head output [mu, v] */
    const float   *mask;                   /* the 144 logits per coarse pixel, addressed through mask_s* */
    const float   *gt;                     /* (B, 4h, 4w) fp32 */
    const uint8_t *valid;                  /* (B, 4h, 4w), 0 / 1 */
    int64_t        mask_sb, mask_sc, mask_sy, mask_sx;
    int64_t        gm_sb, gm_sc, gm_sy, gm_sx;
    float         *pred;                   /* forward, optional: (B, 2, 4h, 4w) [mu, var] */
    double        *sums;                   /* (2): valid count, NLL sum (forward writes, backward reads) */
    float         *loss;                   /* forward: the 0-d loss */
    void          *work;                   /* magnet_dnet_loss_workspace(args) bytes of scratch, forward and backward */
    const float   *grad_loss;              /* backward: device scalar dL/dloss (read on the device) */
    float         *grad_depth;             /* backward: (B, 2, h, w), every element written */
    float         *grad_mask;              /* backward: addressed through gm_s*, 144 channels of every pixel written */
    int32_t        B, h, w, k;             /* k = 4 */
} MagnetDnetLossArgs;
MAGNET_API int64_t magnet_dnet_loss_workspace(const MagnetDnetLossArgs *args);
MAGNET_API int magnet_dnet_loss_forward(const MagnetDnetLossArgs *args, void *stream);
MAGNET_API int magnet_dnet_loss_backward(const MagnetDnetLossArgs *args, void *stream);

/* The plain form, the reference's own call: pred (B, 2, H, W) [mu, var] already upsampled and activated.  The same NLL with var as
 * it is; var < 1e-10 -> 1e-10 (losses.py:19), and a pixel where that clamp applies (var <= 0 included) gets no var gradient.
 * grad_pred: every element written.  work: MAGNET_NLL_BLOCKS * 2 doubles. */
typedef struct MagnetDnetNllArgs {
    const float   *pred;                   /* (B, 2, H, W) fp32 [mu, var] */
    const float   *gt;                     /* (B, H, W) */
    const uint8_t *valid;                  /* (B, H, W), 0 / 1 */
    double        *sums;                   /* (2): valid count, NLL sum (forward writes, backward reads) */
    float         *loss;                   /* forward: the 0-d loss */
    double        *work;                   /* forward: MAGNET_NLL_BLOCKS * 2 doubles of scratch */
    const float   *grad_loss;              /* backward: device scalar dL/dloss (read on the device) */
    float         *grad_pred;              /* backward: (B, 2, H, W) */
    int32_t        B, H, W;
} MagnetDnetNllArgs;
MAGNET_API int magnet_dnet_nll_forward(const MagnetDnetNllArgs *args, void *stream);
MAGNET_API int magnet_dnet_nll_backward(const MagnetDnetNllArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGNET_HIP_H */
