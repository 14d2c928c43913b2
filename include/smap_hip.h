/*
 * smap_hip.h -- C ABI of libsmap_hip.so, the MI355X (gfx950) implementation of
 * the SMAP inference hot path.  Plain pointers and sizes only; no torch types.
 *
 * Every entry point is stream-ordered on the hipStream_t passed as `stream`
 * (void* so that this header needs no HIP include), never allocates, never
 * synchronises, borrows all buffers from the caller and returns
 *      0            on success,
 *      SMAP_E_ARG   (-1) on an argument error,
 *      -(1000+e)    when a HIP call failed with hipError_t e.
 * All pointers are DEVICE pointers unless the parameter says "host".
 *
 * The reference interface each entry replaces is cited as file:line relative
 * to the reference checkout (zju3dv/SMAP).
 */
#ifndef SMAP_HIP_H
#define SMAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations between this push and the pop at the end of the file are its
 * whole dynamic symbol table (tests/test_abi_cpu.py compares `nm -D` with this header in both directions). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define SMAP_E_ARG (-1)

#define SMAP_NJ 15        /* association.cpp:18 nJoints  */
#define SMAP_NL 14        /* association.cpp:19 nLimbs   */
#define SMAP_MAXP 127     /* association.cpp:20 maxPeaks */
#define SMAP_HMS_C 43     /* association.cpp:21 heatmapDim[0] = 15 keypoints + 28 PAF */

/* Library / build identification (also used by the tests to prove the HIP
 * library, not a fallback, is what is loaded). */
const char* smap_version(void);

/* ---- association: replaces extensions/association.cpp::extract/connect ---- */

/* test.py:111-112  hmsIn[:15] /= 255 ; hmsIn[15:] /= 127  (in place, fp32 IEEE divide)
 * hms: [B,43,H,W] fp32. */
int smap_scale_hms(float* hms, int B, int H, int W, void* stream);

/* test.py:55-70 flip-TTA merge, in place on hms [B,43,H,W]: hms[:,i] += s_i * flip_x(hms_flip)[:,pair43[i]]
 * (s_i = -1 on PAF-x channels 15,17,..), then hms[:,15:] *= 0.5.  pair43: HOST pointer to 43 ints
 * (KEYPOINT.FLIP_ORDER followed by 15 + PAF.FLIP_CHANNEL, dataset/data_settings.py:22,33-34). */
int smap_flip_merge(float* hms, const float* hms_flip, const int* pair43, int B, int H, int W, void* stream);

/* nmsBase.cu:10-175 (nmsRegisterKernel + exclusive_scan + writeResultKernel) fused.
 * hms  : [B,C,H,W] fp32, C >= 15 (only channels 0..14 are read)
 * peaks: [B,15,128,3] fp32 out; slot 0 = (count,0,0), slots > count zero-filled.
 * Requires H*W <= 32768. */
int smap_nms(const float* hms, int B, int C, int H, int W, float threshold,
             float* peaks, void* stream);
/* The same result from TWO launches and a caller-provided workspace (the library never allocates): nmsRegisterKernel's mask
 * (nmsBase.cu:10-41) as one thread per pixel over the whole batch -- B x 15 x H x W / 256 workgroups instead of the B x 15 of the
 * fused form, whose 120 workgroups at eight frames walk 26 serial chunks each -- into a bit mask per 64 pixels, then the scan and the
 * 7x7 centroid write-out (nmsBase.cu:43-135, 166) per channel.  workspace: DEVICE memory, 8-byte aligned, at least
 * smap_nms_workspace_bytes(B, H, W) = B * 15 * ceil(H * W / 64) * 8 bytes; not read or written outside the call's launches. */
int64_t smap_nms_workspace_bytes(int B, int H, int W);
int smap_nms_ws(const float* hms, int B, int C, int H, int W, float threshold, float* peaks, void* workspace,
                int64_t workspace_bytes, void* stream);

/* bodyPartConnectorBase.cu:11-63,104-189 (process + pafScoreKernel).
 * hms: [B,43,H,W]; peaks as above; scores: [B,14,127,127] fp32 out (-1 where no pair). */
int smap_paf_score(const float* hms, const float* peaks, int B, int H, int W,
                   float* scores, void* stream);

/* association.cpp:123-233 (findConnectedJoints), batched: one frame per workgroup.
 * rdepth: [B,H,W] fp32 root-depth maps; bodys: [B,127,15,4] fp32 out (x,y,0,score in
 * heat-map pixels; rows >= counts[b] are zero); counts: [B] int32 out. */
int smap_group(const float* peaks, const float* scores, const float* rdepth, int B,
               int H, int W, int root_idx, int dist_flag, float* bodys, int32_t* counts,
               void* stream);

/* test.py:116-134 + test_util.py:45-99 + post_3d.py:4-27 (x4, nearest x4 upsample,
 * generate_relZ, chain_bones, gen_3d_pose, back_projection), batched.
 * det_d : [B,14,H,W] fp32, root_d: [B,H,W] fp32 (heat-map resolution)
 * cams  : [B,9] f64 = scale,img_w,img_h,net_w,net_h,f_x,f_y,cx,cy
 * pred_2d: [B,127,15,4] fp32 out; pred_3d: [B,127,15,4] f64 out; root_z: [B,127] f64 out. */
int smap_lift(const float* bodys, const int32_t* counts, const float* det_d,
              const float* root_d, const double* cams, int B, int H, int W,
              float* pred_2d, double* pred_3d, double* root_z, void* stream);

/* test_util.py:102-131 + refinenet.py:5-37 (lift_and_refine_3d_pose + RefineNet MLP).
 * wt: 5 device pointers (host array) to BN-folded TRANSPOSED weights [in][out] fp32,
 * bs: 5 device pointers (host array) to folded biases [out]; dims 75,160,256,256,128,45.
 * refined: [B,127,15,4] f64 out. */
int smap_refine(const float* pred_2d, const double* pred_3d, const int32_t* counts, int B,
                const float* const* wt, const float* const* bs, double* refined, void* stream);

/* ---- ground-truth modes of test.py (-t generate_result / generate_train), SURVEY.md 8f rank 4 ----
 * register_pred WITH ground truth (test_util.py:18-42), batched: greedy nearest-root matching (< 30 px,
 * ties in row-major (annotation, prediction) order) of connect's persons to the kept annotations.
 * bodys/counts: smap_group's outputs; gt_roots: [B,G,2] fp32 root joint (x,y) of the annotations whose root is
 * visible (test.py:76-80), network pixels; gt_counts: [B] int32 (<= G <= 64).
 * matched: [B,127,15,4] fp32 out -- row g = the prediction assigned to annotation g (heat-map pixels) or zeros;
 * matched_counts: [B] int32 out = gt_counts[b], or 0 when the frame has no prediction / no annotation. */
int smap_register_gt(const float* bodys, const int32_t* counts, const float* gt_roots,
                     const int32_t* gt_counts, int B, int G, float* matched, int32_t* matched_counts,
                     void* stream);

/* smap_lift for those modes: the person array is float64 there (test_util.py:37), so pred_2d is f64 and no
 * intermediate is rounded to fp32; cams carries the annotation's intrinsics (test.py:84-93). */
int smap_lift_gt(const float* bodys, const int32_t* counts, const float* det_d, const float* root_d,
                 const double* cams, int B, int H, int W, double* pred_2d, double* pred_3d, double* root_z,
                 void* stream);

/* smap_lift_gt that also hands out what the Z chain was built from, for the scorer of the maps (smap_evalmaps_update):
 * depth_v: [B,127,14] f64 out, the mean of the ten clamped PAF-Z samples of every sampled limb (generate_relZ's depth_v), 0 elsewhere;
 * bone_mask: [B,127] int32 out, bit k = limb k of the row was sampled (root score > 0 and both of the limb's joints found) -- a
 * sampled depth may be exactly 0.0.  Rows >= counts[b]: zeros, empty mask.  pred_2d / pred_3d / root_z: smap_lift_gt's, bit for bit. */
int smap_lift_gt_bones(const float* bodys, const int32_t* counts, const float* det_d, const float* root_d,
                       const double* cams, int B, int H, int W, double* pred_2d, double* pred_3d, double* root_z,
                       double* depth_v, int32_t* bone_mask, void* stream);

/* smap_refine on the f64 pred_2d of smap_lift_gt. */
int smap_refine_gt(const double* pred_2d, const double* pred_3d, const int32_t* counts, int B,
                   const float* const* wt, const float* const* bs, double* refined, void* stream);

/* refinenet.py:34-37 RefineNet.forward alone: x [N,75] fp32 -> y [N,45] fp32 (same weight format). */
int smap_refine_mlp(const float* x, int N, const float* const* wt, const float* const* bs, float* y,
                    void* stream);

/* dataset/custom_dataset.py:27-68 (cv2.resize(img, (0,0), fx, fy) to fit, centre pad with 128, ToTensor, Normalize) for one
 * image on the device.  src: uint8 [h][w][3] BGR; the resized image is nh x nw = cvRound(h*fy) x cvRound(w*fx) and sits at
 * (top,left) of the net_h x net_w canvas; dst: fp32 [3][net_h][net_w]; mean3/std3: HOST pointers to 3 floats.  The resize is
 * OpenCV's 8-bit INTER_LINEAR restated operation by operation (11-bit fixed-point coefficients, source coordinate
 * (d + 0.5) / f - 0.5, the >>4 / >>16 / +2 >>2 vertical pass; exact 2x shrink = 2x2 box mean). */
int smap_preprocess(const unsigned char* src, int h, int w, int nh, int nw, int top, int left, float* dst,
                    int net_h, int net_w, const float* mean3, const float* std3, double fx, double fy, void* stream);

/* smap_preprocess for a batch whose frames lie in SEPARATE device buffers (no gather copy): frame b of `frames` (a HOST array of B
 * descriptors, copied into the kernel arguments) is written to dst[b] of dst: fp32 [B][3][net_h][net_w], bit for bit what
 * smap_preprocess writes for the same arguments (both run one per-pixel function).  One launch takes SMAP_PREP_MAX_FRAMES frames, a larger
 * B is split into launches of that many on the same stream.  The window may stick out of the canvas on any side -- top / left negative,
 * top + nh > net_h, left + nw > net_w: the crop-and-pad of the annotated sets (dataset/base_dataset.py::croppad_geometry centres it
 * on int((w / 2) * scale), so odd sizes overhang on the right / bottom) -- and is clipped as the host paste clips it; a window wholly off
 * the canvas gives a frame of padding.  h, w are the stored frame's own size: the taps are clamped to it, whatever size nh, nw, fx, fy
 * were derived from.  SMAP_E_ARG: null pointers, B <= 0, non-positive sizes, nh / nw <= 0, fx / fy not positive. */
#define SMAP_PREP_MAX_FRAMES 16
struct smap_prep_frame {
    const unsigned char* src;           /* uint8 [h][w][3] BGR, device */
    int32_t h, w;                       /* stored frame */
    int32_t nh, nw, top, left;          /* resized size and where it sits in the canvas */
    double fx, fy;                      /* the factors given to cv2.resize */
};
int smap_sizeof_prep_frame(void);
int smap_preprocess_batch(const struct smap_prep_frame* frames, int B, float* dst, int net_h, int net_w, const float* mean3,
                          const float* std3, void* stream);

/* ---- training samples: dataset/ImageAugmentation.py aug_rotate + aug_croppad + aug_flip + ToTensor + Normalize in one launch ---- */

/* The 1024 x 16 int16 weight table of OpenCV's 8-bit bicubic remap (INTER_CUBIC, INTER_BITS = 5, INTER_REMAP_COEF_BITS = 15): entry
 * alpha = (fy5 * 32 + fx5) holds the 4 x 4 weights [row][column] of the fractional offset (fx5 / 32, fy5 / 32).  The 1-D float cubic has
 * A = -0.75 and its fourth coefficient is 1 - c0 - c1 - c2; the 2-D weight is saturate_cast<short>(vy * vx * 32768); every entry is
 * forced to sum to 32768 as initInterTab2D does.  Plain host code, no GPU.  out: HOST, 16384 int16.  SMAP_E_ARG: null. */
int smap_cubic_table(int16_t* out);

/* One training sample of smap_augment_batch.  The staged pipeline it stands for: cv2.warpAffine(src, m, (rw, rh), INTER_CUBIC,
 * BORDER_CONSTANT 128) when `rotate`, rounded to uint8; cv2.resize(.., fx, fy) [INTER_LINEAR] of THAT image (rh x rw; the stored frame
 * when rotate == 0) to nh x nw; pasted at (top, left) of the 128-grey canvas (clipped as in smap_preprocess_batch); mirrored in x when
 * `flip`; ToTensor + Normalize.  The rotated image is never written: every linear tap is computed as the 8-bit result of the remap.
 * m: the FORWARD 2 x 3 matrix as handed to cv2.warpAffine (it is inverted here as cv::warpAffine inverts it).  With rotate == 0, m is
 * not read and rh, rw must still be positive (the caller sets them to h, w); with rotate == 0 and flip == 0 the output is byte for byte
 * smap_preprocess_batch's.  h, w, rh, rw are at most SMAP_AUG_MAX_SIDE: NARROWER than OpenCV, whose fixed-point map saturates its
 * coordinates at 16 bits -- no coordinate reaches that saturation here. */
#define SMAP_AUG_MAX_SIDE 16384
struct smap_aug_frame {
    const unsigned char* src;           /* uint8 [h][w][3] BGR, device */
    int32_t h, w;                       /* stored frame */
    int32_t rotate;                     /* 0: no warp (aug_rotate was not called) */
    int32_t rh, rw;                     /* size of the rotated image (nH, nW of rotate_bound) */
    int32_t nh, nw, top, left;          /* resized size and where it sits in the canvas, as in smap_prep_frame */
    int32_t flip;                       /* mirror the canvas in x */
    double m[6];                        /* forward affine matrix, row major */
    double fx, fy;                      /* the factors given to cv2.resize */
};
int smap_sizeof_aug_frame(void);
/* frames: HOST array of B descriptors (copied into the kernel arguments, SMAP_PREP_MAX_FRAMES per launch, a larger B is split on the
 * same stream); dst: fp32 [B][3][net_h][net_w]; mean3 / std3: HOST, 3 floats; cubic_tab: DEVICE copy of smap_cubic_table's output,
 * 16-byte aligned, may be null only if no frame rotates.  SMAP_E_ARG: null pointers, B <= 0, non-positive sizes, fx / fy not positive,
 * a non-finite matrix entry of a rotating frame, a misaligned cubic_tab, any of h, w, rh, rw above SMAP_AUG_MAX_SIDE. */
int smap_augment_batch(const struct smap_aug_frame* frames, int B, float* dst, int net_h, int net_w, const float* mean3,
                       const float* std3, const int16_t* cubic_tab, void* stream);

/* ---- backbone: replaces model/smap.py SMAP.forward (eval) ------------------ */

/* One op of the static inference schedule.  Offsets are BYTE offsets into the
 * caller's activation arena / weight blob; -1 = absent. */
enum smap_op_kind {
    SMAP_OP_CONV = 0,       /* conv_bn_relu (smap.py:13-45) with folded BN, implicit GEMM on MFMA; with tail_cout / head_cin a
                               Bottleneck's 3x3 + 1x1, or the whole Bottleneck (smap.py:48-77), in one launch */
    SMAP_OP_STEM = 1,       /* ResNet_top conv 7x7 s2 (smap.py:83-84) from fp32 NCHW input      */
    SMAP_OP_MAXPOOL = 2,    /* ResNet_top maxpool 3x3 s2 p1 (smap.py:86)                         */
    SMAP_OP_UPADD = 3,      /* out = relu(a + bilinear_align_corners(t)) (smap.py:213-217)       */
    SMAP_OP_HEADSUM = 4,    /* fp32 NCHW out = sum of bilinear-upsampled heads (smap.py:221-229,417-419) */
    SMAP_OP_STEMPOOL = 5,   /* ResNet_top whole (smap.py:83-86): STEM followed by MAXPOOL in one kernel; H,W = image,
                               Ho,Wo = pooled size, same weight format as STEM                                  */
    SMAP_OP_TAPSUM = 6,     /* the second half of a 3x3 conv with ONE output channel whose first half ran inside the producing launch
                               (CONV with tap_n = 9): out[b,0,y,x] = bias + sum over (dy,dx) in {-1,0,1}^2 of t[b, y+dy, x+dx][3 (dy+1) + dx+1]
                               (zero outside the map) -- fp32 NCHW map at ext_off of the output buffer, like HEADSUM (same status words).
                               aux_off[0] = t, fp32 [B,H,W,Cin] (Cin = 16: nine used); Ho,Wo = H,W; Cout = 1; bias: one fp32 at bias_off */
};

typedef struct smap_op {
    int32_t kind;
    int32_t B, H, W, Cin;           /* input geometry (CONV/MAXPOOL/UPADD: NHWC fp16; STEM: NCHW fp32) */
    int32_t in_stride_c, in_c_off;  /* CONV: channel stride / first channel of the input pixel   */
    int32_t Ho, Wo, Cout;           /* output geometry                                           */
    int32_t ksize, stride, pad;
    int32_t relu;                   /* apply ReLU after bias (+residual)                         */
    int32_t cout_pad;               /* rows of the padded weight matrix (multiple of the N tile) */
    int32_t out_stride_c;           /* channel stride of the output pixel (>= Cout)              */
    int32_t out_c_off;              /* channel offset inside the output pixel                    */
    int32_t out_fp32;               /* CONV: 1 = fp32 NHWC output (heads), 0 = fp16              */
    int32_t tile;                   /* CONV tile selector: 0=128x128 1=128x64 2=64x64 3=128x32 4=64x128 */
    int32_t n_aux;                  /* HEADSUM: number of source tensors (1..3)                  */
    int64_t in_off, out_off;        /* arena byte offsets                                        */
    int64_t w_off, bias_off;        /* weight-blob byte offsets.  CONV: fp16 weights of [cout_pad][K], K = (kh, kw, cin), stored
                                       as ONE CONTIGUOUS BLOCK PER STAGED WEIGHT TILE in the kernel's LDS order, so that
                                       every wave-wide LDS-DMA reads one contiguous KiB (strided 64-byte row segments
                                       stream from L2 at half the rate):
                                         [n tile][K tile][plane][BN rows][16-byte slots]
                                       BN = the N extent of `tile` (smap_conv_tile_dims), K tile = smap_conv_tile_bk(tile,
                                       precision) halves in K order, slot s of row r = K granule s ^ ((r>>1)&7) (64-half
                                       tiles) or s ^ ((r>>2)&3) (32-half tiles; with w_pairs = 1 those are stored in PAIRS,
                                       [n tile][pair][plane][BN rows][tile 2p (64 B) | tile 2p+1 (64 B)]: 128-byte rows); halo tiles 30..49: blocks ordered
                                       [n tile][channel chunk][tap], 128-byte rows of 64 channels (precision 1: of 32
                                       channels as granules 0..3 = hi, 4..7 = lo), slot s = granule s ^ ((r>>1)&7).
                                       Reference packer: smap_amd/engine.py::pack_conv_weights.  + fp32 bias [cout_pad].
                                       STEM: fp16 [64][176] with K = (kh, c, kw padded to 8) + 8 zero columns, + fp32 [64] */
    int64_t res_off;                /* dense [M][Cout] tensor added before ReLU, or -1           */
    int64_t add1_off, add2_off;     /* dense tensors added AFTER ReLU (smap.py:142-153), or -1   */
    int64_t aux_off[3];             /* CONV: aux[0] = optional low-res fp16 [B,aux_h,aux_w,Cout] tensor, bilinearly
                                       (align_corners) upsampled and added before ReLU (smap.py:213-217);
                                       UPADD: aux[0] = low-res t [B,aux_h,aux_w,Cout] (in_off / out_off: [B,Ho,Wo,Cout]), required;
                                       HEADSUM: n_aux fp32 NHWC head tensors (arena) of [B (2 B with flip_from),aux_h,aux_w,Cin], required */
    int32_t aux_h[3], aux_w[3];     /* their spatial sizes                                       */
    int64_t ext_off;                /* HEADSUM: byte offset of the [B,Cout,Ho,Wo] block in the fp32 output buffer */
    int32_t precision;              /* CONV/STEM/MAXPOOL: 0 = fp16 activations and weights (one rounding per stored value,
                                       ~1e-3 relative error through the 200-layer graph); 1 = SPLIT precision, the mode
                                       that reproduces the reference's fp32 arithmetic (smap.py runs fp32 end to end):
                                       every fp16 tensor is stored as two planes, pixel = [hi(C) | lo(C)] with
                                       hi = fp16(v), lo = fp16(v - hi) (in_stride_c / out_stride_c are then 2*C and
                                       res/add/aux tensors have pixel stride 2*Cout8); weights are two consecutive
                                       matrices hi | lo of (w * 2^s); three MFMAs per K step (hi*hi + hi*lo + lo*hi)
                                       into fp32.  fp32 head outputs (out_fp32) and HEADSUM are the same in both modes. */
    float acc_scale;                /* precision 1: 2^-s, applied to the accumulator before the bias             */
    int32_t flip_from;              /* flip-TTA inside the schedule (test.py:55-70), 0 = off.  STEM: frames b >= flip_from
                                       are computed from the x-MIRRORED image of input frame b - flip_from (the input
                                       holds flip_from frames, the schedule runs B = 2 * flip_from).  HEADSUM: B is the
                                       number of OUTPUT frames; when flip_from > 0 the summed maps of frame b + flip_from
                                       are merged into frame b: out[b,c,y,x] = v[b,c,y,x] + s_c * v[b+flip_from, pair[c], y,
                                       W-1-x], s_c = -1 on PAF-x channels (c >= in_c_off, (c - in_c_off) even), then
                                       channels >= in_c_off are halved; pair = int32[Cout] at w_off in the weight blob.
                                       HEADSUM: Cin (the sources' channel stride) is a multiple of 4, every aux_h / aux_w below n_aux
                                       is >= 1, and flip_from is 0 or B. */
    int32_t w_pairs;                /* CONV, 32-half K tiles only: 1 = the weight blob stores them in pairs (see w_off), 0 = one
                                       contiguous block per K tile */
    int32_t status_off;             /* HEADSUM: byte offset (> 0) in the fp32 output buffer of SMAP_STATUS_WORDS(B) int32 STATUS words, or
                                       0 = none.  smap_plan_run clears them; when a value the head sum writes for output frame b is not
                                       finite it ORs bit 0 and bit 1 + b % 31 into word b / 31, and bit 0 into word 0 (so word 0's bit 0
                                       says "some frame of the launch", and a host can drop exactly the affected frames of a launch of
                                       any size and keep the others): split precision keeps
                                       fp16's RANGE, an activation beyond 65504 turns into inf / NaN downstream; the host
                                       checks the word when it collects the maps. */
    int32_t tail_cout;              /* CONV, tile ids 80..89 only (else 0): the op is a Bottleneck TAIL in one launch
                                       (smap.py:48-77) -- a 3x3 stride-1 conv Cin -> Cout (= the tile's N extent, bias + ReLU,
                                       never stored) followed by a 1x1 conv Cout -> tail_cout whose bias / res_off / relu /
                                       add1_off / add2_off / out_* fields are this op's: the output tensor has tail_cout
                                       channels (multiple of 8).  0 = a plain conv. */
    int32_t tail_cout_pad;          /* rows of the padded 1x1 weight matrix: multiple of smap_conv_tile_tail_bn(tile) */
    float tail_acc_scale;           /* precision 1: 2^-s of the 1x1 weights */
    int64_t tail_w_off;             /* weight-blob byte offsets of the 1x1: blocks [n chunk][k chunk][BN2 rows][128 B], rows */
    int64_t tail_bias_off;          /* in the halo tiles' format (64 channels, or hi32 | lo32); fp32 bias [tail_cout_pad] */
    int32_t head_cin;               /* CONV, tile ids 90..99 only (else 0): the op is a WHOLE stride-1 identity Bottleneck in one launch
                                       (smap.py:48-77; csrc/convb.hip: Cin = 64 planes, tile ids 90..93; csrc/convc.hip: 128 planes, tile id 94;
                                       split precision): a LEADING 1x1 conv head_cin -> Cin (bias +
                                       ReLU, never stored, recomputed on the 3x3's halo) in front of the 3x3 and its tail.  The input
                                       tensor then has head_cin channels (in_stride_c = 2 * head_cin), is read once, and is also
                                       the residual: res_off must equal in_off and tail_cout = head_cin. */
    float head_acc_scale;           /* 2^-s of the leading 1x1's weights */
    int64_t head_w_off;             /* weight-blob byte offsets of the leading 1x1: blocks [k chunk][Cin rows][128 B] in the halo */
    int64_t head_bias_off;          /* tiles' row format (hi32 | lo32 of 32 input channels: tile ids 92..94; tile ids 90, 91: 16-channel stages, 64-byte rows,
                                       smap_amd/engine.py::pack_rows16); fp32 bias [Cin] */
    int64_t short_w_off;            /* tile ids 92, 93 only (present iff short_acc_scale > 0): the FIRST block of a layer (smap.py:124-129) -- head_cin = 64 input
                                       channels and, instead of "+ input", a 1x1 SHORTCUT conv head_cin -> tail_cout (folded BN, no ReLU) on
                                       the same input, added before the final ReLU.  Weight blocks [n chunk][k chunk][64 rows][128 B] like
                                       the tail's; its bias is folded into the tail's bias by the packer; res_off = -1 */
    float short_acc_scale;          /* 2^-s of the shortcut conv's weights; 0 = the op has no shortcut conv */
    int32_t scale_hms;              /* HEADSUM: 1 = the maps are written ALREADY SCALED as exps/stage3_root2/test.py:111-112 scales them before the
                                       association: channels < in_c_off (the key points) / 255, the others (the PAFs) / 127 -- the same fp32
                                       divisions smap_scale_hms performs, applied to the summed (and, with flip_from, merged) value in the
                                       head sum's store, so that no separate pass over the maps runs between the backbone and smap_nms.
                                       0 = raw maps: what model.smap.SMAP.forward returns (smap.py:417-419).  Other kinds: 0. */
    /* N SEGMENTS: several 1x1 convs that read the SAME input as one launch with up to three outputs (Upsample_unit, smap.py:210-241:
       u_skip and skip1 both read x; skip2, cross_conv / res_conv1 and the next unit's up_conv all read `out`).  The weight
       matrix [cout_pad][K] is the concatenation of the convs' rows, every segment starting on a multiple of the tile's N extent
       (rows in between are zero); segment 0 = rows [0, seg_n[0]) is described by the op's own fields (Cout, out_off, relu,
       acc_scale, res / add / aux: those apply to segment 0 only); segment j = 1, 2 = rows [seg_n[j-1], seg_n[j] or cout_pad)
       writes seg_cout[j-1] channels (multiple of 8) to the dense fp16 tensor at seg_out_off[j-1] (channel stride
       seg_out_stride_c[j-1]) with its own ReLU flag and accumulator scale.  seg_n[0] = 0: a plain conv.  Tile ids of
       csrc/conv.hip only (0..9, 20..27, 50..55), ksize 1, fp16 outputs. */
    int32_t seg_n[2];
    int32_t seg_cout[2], seg_relu[2], seg_out_stride_c[2];
    float seg_acc_scale[2];
    int64_t seg_out_off[2];
    /* SPLIT K (tile ids 2, 7, 20, 22 of csrc/conv.hip; small schedules -- batch 1 -- whose launches have fewer output tiles than the chip has
       CUs): ksplit = S > 1 workgroups per output tile, each over 1/S of the K tiles; their raw fp32 accumulators meet in the scratch
       area at kpart_off (arena bytes: m_tiles * n_tiles * S * BM * BN * 4, BM x BN = smap_conv_tile_dims) and the last workgroup to
       arrive -- one uint32 ticket per tile at kcount_off (arena; smap_plan_run zeroes the tickets of a schedule before its first op,
       the kernel leaves them at zero) -- sums the parts in the fixed order 0 .. S-1 and runs the epilogue: deterministic, one launch.
       0 or 1 = off.  S <= 16 and S <= the number of K tiles (K / smap_conv_tile_bk). */
    int32_t ksplit, reserved1;
    int64_t kpart_off, kcount_off;
    /* LANES (smap_plan_set_lanes): independent branches of the schedule -- the head chains of an Upsample_unit (model/smap.py:219-229)
       next to the unit that follows -- may run on forked streams.  lane = 0 (the caller's stream) .. SMAP_MAX_LANES - 1; wait_op = indices
       of EARLIER ops on OTHER lanes whose results this op reads (-1 = unused; n_wait of them).  smap_plan_run makes the op's stream wait
       for those ops and joins every lane into the caller's stream at the end; inside a stream capture the lanes become parallel branches
       of the graph.  With lanes off (the default) every op runs on the caller's stream in order and the fields are ignored.  The packer
       guarantees that buffers touched by an op on a side lane are not reused before the end of the schedule. */
    int32_t lane, n_wait;
    int32_t wait_op[4];
    /* SECOND INPUT, concatenated along K (round 6; csrc/conv.hip tiles 20, 50, 51, 53, 54; ksize 1): the op computes
           out = act( W [x | x2_sampled] + bias (+ res) )
       -- ONE accumulator over K = Cin + in2_C, the weight matrix [cout_pad][Cin + in2_C] being the two convs' matrices side by side.  This is
       the last 1x1 of a stride-2 / widening Bottleneck TOGETHER with its 1x1 shortcut conv (model/smap.py:60-77, 124-129:
       out = relu(bn3(conv3(y)) + downsample(x)), no activation between the two sums): the shortcut's output is never written or read back and
       its launch disappears.  x2 = fp16 NHWC tensor [B, in2_H, in2_W] of in2_C channels (channel stride in2_stride_c, hi | lo planes in split
       precision like every tensor) at in2_off, sampled at pixel (oy * in2_stride, ox * in2_stride) for output pixel (oy, ox):
       Ho = (in2_H - 1) / in2_stride + 1, likewise Wo.  in2_C = 0: no second input.  x2 lies in the same 4 GiB window as the first input
       (one 64-bit base per launch, include/smap_hip.h "windows").  Not with split K, N segments, the fused bilinear add or a 3x3. */
    int64_t in2_off;
    int32_t in2_H, in2_W, in2_C, in2_stride_c, in2_stride;
    /* in2_mode = 1 (needs in2_C > 0, in2_stride = 1): NOT one sum over the concatenated K but the sum of two ACTIVATED convs,
           out = relu(W1 x + b1) + relu(W2 x2 + b2),
       in one launch: the K loop walks x's tiles, the accumulators are turned into relu(acc * acc_scale + bias) and parked in registers, then
       it walks x2's tiles from zero.  The inter-stage skips of an Upsample_unit, skip1(x) + skip2(out) (smap.py:218-241, 142-153: both are only
       ever ADDED to the next stage's feature map), as ONE tensor: one write and one read of an in_planes-wide tensor less per level.  The
       packed weight matrix is [W1 2^s1 | W2 2^s2] along K; bias_off / acc_scale belong to W1, in2_bias_off / in2_acc_scale to W2; the op's
       relu field is ignored.  in2_mode = 0: the K-concatenated sum described above. */
    int32_t in2_mode;
    float in2_acc_scale;
    int64_t in2_bias_off;
    /* TAP-DOT EPILOGUE (round 6; csrc/conv.hip tile 54 = 128 x 256, cout_pad = 256 = ONE N tile, ksize 1): tap_n = 9 -- the launch's
       activation y = act(W x + b) is NOT stored; its only consumer is a 3x3 conv with one output channel (smap.py:227-229, res_rd_conv2 on
       res_rd_conv1), whose per-pixel half the epilogue computes instead, on the matrix cores: t[m][k] = < tapw[k], y[m] >, k = 0..8.
       tapw at tap_w_off in the weight blob: the folded 3x3 weights [kh*3+kw][channel] * 2^s as fp16 hi | lo in the B-fragment order of
       v_mfma_f32_16x16x32_f16 -- [K step 0..7][plane hi, lo][lane 0..63][8 halves], lane l holding tap l % 16 (taps 9..15: zeros), channels
       32 step + 8 (l / 16) .. +7 -- and tap_scale = 2^-s.  `out` is then the fp32 tensor t, pixel stride out_stride_c = 16 (out_fp32 = 1,
       entries 9..15 written as zeros), and a TAPSUM op finishes the conv.  0 = off.  Not with res / adds / segments / split K / in2. */
    int32_t tap_n;
    float tap_scale;
    int64_t tap_w_off;
} smap_op;

#define SMAP_STATUS_WORDS(frames) (((frames) + 30) / 31)      /* int32 status words of a schedule with `frames` output frames */

/* sizeof(smap_op) as compiled: lets a foreign-language binding verify its struct mirror. */
int smap_sizeof_op(void);
/* Geometry of a CONV tile id, for whoever packs the weight blob: M x N extent of the output tile (0 on success, -1 for an
 * unknown id) and the halves per staged K tile for `precision` (0 for an unknown id). */
int smap_conv_tile_dims(int tile, int* bm, int* bn);
int smap_conv_tile_bk(int tile, int precision);
/* Tile ids with a fused 1x1 tail (80..89: 3x3 + tail; 90..99: whole Bottleneck): output channels per chunk of the tail (its weight
 * rows are padded to a multiple); 0 for every other id. */
int smap_conv_tile_tail_bn(int tile);

typedef struct smap_plan smap_plan;
#define SMAP_MAX_LANES 4

/* Copies `ops`; validates geometry.  n_ops <= 4096.  Arena contract: the conv kernels address their input with a 64-bit
 * base (the input's WINDOW: its arena offset rounded down to a multiple of 4 GiB) plus 32-bit lane offsets, and read zeros
 * for padding taps at the start of that window.  So bytes [k * 2^32, k * 2^32 + 16384) are RESERVED for every k >= 0
 * (smap_plan_run zeroes the ones its launches use), no tensor overlaps them (hence no tensor crosses a 4 GiB boundary and
 * none exceeds 4 GiB - 16 KiB), and the arena may be of any size.  This holds for EVERY arena range of EVERY op kind -- in_off /
 * out_off of MAXPOOL and UPADD, out_off of STEM and STEMPOOL, UPADD's aux_off[0], the n_aux sources of a HEADSUM, TAPSUM's aux_off[0],
 * a CONV's second input, segment outputs and split-K scratch and tickets: each is required (>= 16384; -1 = absent only for res_off,
 * add1_off, add2_off and aux_off[0] of a CONV).  A split-K ticket slice shares no byte with any other arena range of the schedule.
 * Weight-blob offsets of the operands an op uses are >= 0; a size that does not fit int64 makes the op invalid. */
int smap_plan_create(const smap_op* ops, int n_ops, smap_plan** plan);
void smap_plan_destroy(smap_plan* plan);
/* Runs the whole schedule on `stream`.
 * input : [B,3,H,W] fp32 NCHW images; arena: activation arena; weights: weight blob;
 * out   : fp32 output buffer (hms [B,43,h,w] | det_d [B,14,h,w] | root_d [B,1,h,w] at the
 *         offsets recorded in the HEADSUM ops, plus the SMAP_STATUS_WORDS(B) int32 status words at status_off when the ops name them). */
int smap_plan_run(const smap_plan* plan, const float* input, void* arena, const void* weights,
                  float* out, void* stream);
/* The same with the images in n_inputs (1..SMAP_MAX_INPUTS, a divisor of B) separate buffers of B / n_inputs frames each,
 * in order: `inputs` is a HOST array of device pointers.  A launch that serves several of the caller's batches reads them
 * where they are (the stem indexes the buffers) instead of gathering them first (test.py:43-50 hands one batch at a time). */
#define SMAP_MAX_INPUTS 8
int smap_plan_run_inputs(const smap_plan* plan, const float* const* inputs, int n_inputs, void* arena,
                         const void* weights, float* out, void* stream);
/* Lanes on (1) / off (0, the default): see smap_op.lane.  Switching them on creates the side streams and events IN THIS CALL, on the current
 * device (all or nothing: a failure is this call's return code and leaves nothing behind); they are destroyed with the plan.  smap_plan_run
 * never creates anything (a first run inside a stream capture is fine) and joins the side lanes into the caller's stream on error returns
 * too.  A plan with lanes ON has one caller at a time -- its side streams are shared by whoever runs it; with lanes off a plan is immutable
 * and may be run from several host threads / executors at once. */
int smap_plan_set_lanes(smap_plan* plan, int on);
/* Bytes of arena and of output buffer the schedule touches, computed from the ops (either pointer may be NULL). */
int smap_workspace_bytes(const smap_plan* plan, int64_t* arena_bytes, int64_t* out_bytes);

/* ---- plan blob: the whole schedule as ONE relocatable byte image, so that a host that cannot run the Python schedule builder
 * (smap_amd/engine.py describes model/smap.py:313-353 as ops and packs the weights) can still run SMAP.forward from this header
 * alone: read the file, smap_plan_create_from_blob, hipMalloc info.arena_bytes / info.out_bytes, upload the blob's weight
 * section [weights_offset, +weights_bytes) to the device, smap_plan_run.  Little-endian, written by
 * smap_amd/engine.py::BackboneEngine.blob():
 *   smap_blob_header | smap_op[n_ops] at ops_offset | weight section at weights_offset (256-byte aligned) */
#define SMAP_BLOB_VERSION 2u
typedef struct smap_blob_info {
    int32_t frames, H, W;               /* input: [frames,3,H,W] fp32 NCHW                                      */
    int32_t out_h, out_w;               /* map size                                                              */
    int32_t n_hms, n_det, n_root;       /* channels of the three outputs (43, 14, 1)                             */
    int32_t precision;                  /* 0 = fp16 storage, 1 = split precision                                 */
    int32_t reserved;
    int64_t arena_bytes, out_bytes;     /* buffers to allocate (out_bytes includes the status word)              */
    int64_t weights_offset, weights_bytes;   /* the weight section inside the blob                               */
    int64_t hms_off, det_off, root_off, status_off;   /* byte offsets of [frames,C,out_h,out_w] fp32 maps / the int32 status word in `out` */
} smap_blob_info;
typedef struct smap_blob_header {
    char magic[8];                      /* "SMAPPLN1"                                                            */
    uint32_t version, sizeof_op, header_bytes;   /* version = SMAP_BLOB_VERSION: any other value is refused (a blob written for an older smap_op
                                           MEANING -- version 1: status_off named ONE status word, no seg_ / ksplit / lane / scale_hms
                                           fields -- must not load just because the struct sizes happen to agree) */
    int32_t n_ops;
    int64_t ops_offset;
    int64_t weights_offset, weights_bytes, arena_bytes, out_bytes;     /* = info's, kept flat for readers without the struct */
    smap_blob_info info;
} smap_blob_header;
/* blob: HOST memory.  Validates header, op size, every op (as smap_plan_create) and that the ops stay inside the arena /
 * output sizes the header states.  info may be NULL. */
int smap_plan_create_from_blob(const void* blob, size_t blob_bytes, smap_plan** plan, smap_blob_info* info);

/* Runs ops [first, first+count) only (tests, per-layer profiling). */
int smap_plan_run_range(const smap_plan* plan, int first, int count, const float* input,
                        void* arena, const void* weights, float* out, void* stream);

/* ---- JPEG decode: replaces the image decode of dataset/custom_dataset.py (cv2.imread; here PIL + EXIF transpose) ----
 *
 * Split at the natural seam: the HOST (csrc/jpeg_host.cpp, plain C++, no HIP, no global state, safe to call from many threads at once)
 * parses the markers and Huffman-decodes the entropy-coded data into quantised coefficients; the GPU (csrc/jpeg.hip) dequantises,
 * runs libjpeg's ISLOW inverse DCT, upsamples the chroma ("fancy", as libjpeg does by default), converts YCbCr to BGR and applies
 * the EXIF orientation -- bit for bit what libjpeg-turbo + PIL's exif_transpose hand the network (DESIGN.md "JPEG decode").
 * Supported: 8-bit baseline / extended sequential Huffman, one interleaved scan, grey or YCbCr with luma sampling 1x1, 2x1 or 2x2
 * and chroma 1x1 (4:4:4, 4:2:2, 4:2:0), restart intervals, EXIF orientation 1-8.  Anything else valid is SMAP_JPEG_UNSUPPORTED
 * (the caller decodes it with PIL); malformed data is SMAP_JPEG_E_DATA (the caller also falls back, and PIL then raises). */
#define SMAP_JPEG_UNSUPPORTED 1
#define SMAP_JPEG_E_DATA (-2)

typedef struct smap_jpeg_info {
    int32_t width, height;              /* as stored (before the orientation)                                          */
    int32_t orientation;                /* EXIF orientation 1-8 (1 = none; out-of-range values count as 1, as in PIL)   */
    int32_t ncomp;                      /* 1 (grey) or 3 (YCbCr)                                                       */
    int32_t h_samp[3], v_samp[3];       /* sampling factors (grey: 1, 1)                                               */
    int32_t blocks_w[3], blocks_h[3];   /* 8x8 blocks per line / per column of each component, MCU padding included    */
    uint16_t quant[3][64];              /* quantisation table of each component, NATURAL order                        */
    int64_t coef_offset[3];             /* byte offset of each component's coefficient plane                          */
    int64_t coef_bytes;                 /* all planes: int16 [component][block row][block col][64], natural order     */
    int64_t scan_offset;                /* byte offset of the entropy-coded data in the file                          */
    int32_t restart_interval;           /* MCUs per restart interval, 0 = none                                        */
    int32_t reserved;
} smap_jpeg_info;

/* sizeof(smap_jpeg_info) as compiled (binding check, as smap_sizeof_op). */
int smap_sizeof_jpeg_info(void);

/* data: HOST bytes of a whole file.  Parses the markers up to the first SOS.  0 = supported (info filled), SMAP_JPEG_UNSUPPORTED,
 * SMAP_JPEG_E_DATA or SMAP_E_ARG. */
int smap_jpeg_probe(const uint8_t* data, size_t n, smap_jpeg_info* info);

/* data / info / coeffs: HOST.  info must be what smap_jpeg_probe returned for these bytes.  Writes info->coef_bytes of QUANTISED
 * coefficients (absolute DC, natural order, every block of the MCU grid).  Any surprise in the entropy-coded data -- a bad code, an
 * early marker or end of file, a wrong RSTn, data left over after the last MCU -- is SMAP_JPEG_E_DATA. */
int smap_jpeg_decode_coefficients(const uint8_t* data, size_t n, const smap_jpeg_info* info, int16_t* coeffs);

/* Device scratch smap_jpeg_reconstruct needs for the component planes (bytes; = coef_bytes / 2).  info: HOST. */
int64_t smap_jpeg_workspace_bytes(const smap_jpeg_info* info);

/* coeffs: DEVICE copy of smap_jpeg_decode_coefficients' output; info: HOST; planes: DEVICE scratch of smap_jpeg_workspace_bytes;
 * bgr: DEVICE uint8 [H'][W'][3], the orientation applied (orientations 5-8 swap width and height).  Two launches on `stream`. */
int smap_jpeg_reconstruct(const int16_t* coeffs, const smap_jpeg_info* info, uint8_t* planes, uint8_t* bgr, void* stream);

/* ---- Huffman decode on the device (csrc/jpeg_huff.h, csrc/jpeg_huff.hip; DESIGN.md "JPEG decode", "Huffman decode on the GPU") ----
 * The host parses the markers and packs the scan's Huffman tables (microseconds); the GPU decodes the entropy-coded segment into the
 * coefficients smap_jpeg_decode_coefficients writes: subsequences of the segment are decoded speculatively, one per lane, their decoder
 * states are propagated to a fixed point, and a last EXACT pass re-decodes from those states, repeats every check of the host decoder
 * and verifies that the chain of states closes.  Only that pass is trusted: status 0 means its output is the host decoder's. */
#define SMAP_JPEG_DEV_E_DATA 1            /* the exact pass met what smap_jpeg_decode_coefficients calls SMAP_JPEG_E_DATA          */
#define SMAP_JPEG_DEV_NOT_CONVERGED 2     /* the chain of decoder states did not close (more rounds, or the host decoder)         */
#define SMAP_JPEG_SUBSEQ_BYTES 128        /* shipped defaults of subseq_bytes and rounds (DESIGN.md has the runs behind them)     */
#define SMAP_JPEG_ROUNDS 8
#define SMAP_JPEG_MAX_MCU_BLOCKS 6        /* 2x2 luma + Cb + Cr                                                                    */

/* One Huffman table in decoding form: a 9-bit lookahead, then jdhuff.c's maxcode / valoff / vals for the longer codes. */
typedef struct smap_jpeg_huff {
    uint16_t look[512];                 /* (code length << 8) | symbol; 0 = longer than 9 bits, or no such code              */
    int32_t maxcode[18];                /* largest code of each length, -1 = none; [17] = INT32_MAX                          */
    int32_t valoff[18];                 /* index into vals of the first code of each length, minus that code                */
    uint8_t vals[256];
} smap_jpeg_huff;

typedef struct smap_jpeg_scan {
    smap_jpeg_huff table[6];            /* [2 * c] = DC table of scan component c, [2 * c + 1] = its AC table                */
    int32_t ncomp;
    int32_t blocks_per_mcu;
    int32_t block_comp[SMAP_JPEG_MAX_MCU_BLOCKS];   /* of each block of the MCU, in scan order: its component ...            */
    int32_t block_v[SMAP_JPEG_MAX_MCU_BLOCKS];      /* ... and its (v, h) inside the component's part of the MCU             */
    int32_t block_h[SMAP_JPEG_MAX_MCU_BLOCKS];
    int32_t restart_interval;
    int32_t reserved;
    int64_t scan_offset;                /* as smap_jpeg_info                                                                */
    int64_t file_bytes;
    int64_t total_blocks;               /* every block of the MCU grid, all components                                      */
} smap_jpeg_scan;

/* sizeof(smap_jpeg_scan) as compiled (binding check). */
int smap_sizeof_jpeg_scan(void);

/* data / info / scan: HOST.  Fills `scan` for these bytes; the refusals of smap_jpeg_decode_coefficients at the marker level (info is
 * not this file's: SMAP_E_ARG; an undefined table, an over-long code set, a DC category above 15: SMAP_JPEG_E_DATA).  No allocation,
 * no global state, callable from many threads. */
int smap_jpeg_scan_tables(const uint8_t* data, size_t n, const smap_jpeg_info* info, smap_jpeg_scan* scan);

/* Device scratch of smap_jpeg_decode_coefficients_device (bytes; 0 = bad arguments).  subseq_bytes: 0 = SMAP_JPEG_SUBSEQ_BYTES, else a
 * multiple of 4 in 8..128.  info: HOST. */
int64_t smap_jpeg_huff_workspace_bytes(const smap_jpeg_info* info, size_t file_bytes, int subseq_bytes);

/* d_file: DEVICE copy of the whole file; info: HOST, what smap_jpeg_probe returned for it; d_scan: DEVICE copy of what
 * smap_jpeg_scan_tables filled (8-byte aligned); rounds: cross-workgroup propagation launches, 0 = SMAP_JPEG_ROUNDS, at most the number
 * of workgroups = ceil(ceil((file_bytes - scan_offset) / subseq_bytes) / 256), which is provably enough for any valid file; workspace:
 * DEVICE, 8-byte aligned.  d_coeffs: DEVICE, info->coef_bytes, the layout of smap_jpeg_decode_coefficients.  *d_status (DEVICE) is
 * 0 -- d_coeffs is bit for bit what smap_jpeg_decode_coefficients writes for these bytes -- or an OR of SMAP_JPEG_DEV_E_DATA and
 * SMAP_JPEG_DEV_NOT_CONVERGED: the caller then uses the host decoder.  A fixed sequence of launches on `stream`, no read-back. */
int smap_jpeg_decode_coefficients_device(const uint8_t* d_file, size_t file_bytes, const smap_jpeg_info* info,
                                         const smap_jpeg_scan* d_scan, int subseq_bytes, int rounds, void* workspace,
                                         int64_t workspace_bytes, int16_t* d_coeffs, int32_t* d_status, void* stream);

/* ---- scoring: lib/eval/test_util_panoptic.py eval_3d (:273-307), initialization (:332-355) on the device ----
 * The accumulator is SMAP_EVAL_ACC_DOUBLES f64 on the device, kept across calls:
 *   real_error[15] | root_error[15] | count_point[15] | real_PCK[15] | root_PCK[15] |
 *   count_people, total_people_gt, total_pair_count, reverse_pair_count, less_15.
 * A person's term row has the SAME layout: field f of the row is what eval_3d adds to accumulator field f for that person
 * (0 where the reference adds nothing: x + 0.0 == x for every x the sums can hold, which are never -0.0). */
#define SMAP_EVAL_ACC_DOUBLES 80
#define SMAP_EVAL_TERM_DOUBLES 80
#define SMAP_EVAL_MAXG 64

/* acc = zeros, total_pair_count = 1e-8 (:351). */
int smap_eval3d_acc_init(double* acc, void* stream);

/* The per-person part of eval_3d, parallel over (frame, person, joint).
 * pred_3d: [B,127,15,4] f64 (smap_lift_gt / smap_refine_gt layout); counts: [B] int32, persons of the frame = its kept annotations
 * (values outside 0..G are clamped); gt: [B,G,15,4] f64 = (X,Y,Z,score) of the kept annotations (columns 4:7 and 3 of the annotation
 * rows), 1 <= G <= SMAP_EVAL_MAXG.  terms: [B,G,SMAP_EVAL_TERM_DOUBLES] f64 out.  Rows >= counts[b] of pred_3d, gt and terms are
 * neither read nor written.  float64 without contraction, correctly rounded square root: bit for bit numpy's. */
int smap_eval3d_terms(const double* pred_3d, const int32_t* counts, const double* gt, int B, int G, double* terms, void* stream);

/* The ordered part: acc[f] += terms[b][g][f] for b = 0..B-1, g = 0..counts[b]-1 IN THAT ORDER, one thread per field -- the
 * reference's running sums, person by person (a per-frame partial sum would re-associate the float64 additions). */
int smap_eval3d_fold(const double* terms, const int32_t* counts, int B, int G, double* acc, void* stream);

/* Both parts on `stream`: ONE launch (a single workgroup computes the terms, then folds them) while B * G <= 1024, otherwise
 * smap_eval3d_terms followed by smap_eval3d_fold.  Same bits either way.  terms: caller's scratch [B,G,SMAP_EVAL_TERM_DOUBLES]. */
int smap_eval3d_update(const double* pred_3d, const int32_t* counts, const double* gt, int B, int G, double* terms, double* acc,
                       void* stream);

/* ---- scoring the maps: eval_one_image (:88-113) and the `eval` part of generate_rootZ (:145-156) on the device ----
 * The accumulator is SMAP_EVALMAPS_ACC_DOUBLES f64, kept across calls:
 *   count_gt[15] | count_pred[15] | distance_e[15] | distance_d[14] | reverse_count[14] | count_pred_bone[14];
 * a person's term row has the same layout. */
#define SMAP_EVALMAPS_ACC_DOUBLES 87

/* acc = zeros. */
int smap_evalmaps_acc_init(double* acc, void* stream);

/* pred_2d: [B,127,15,4] f64 and depth_v [B,127,14] f64 / bone_mask [B,127] int32 as smap_lift_gt_bones wrote them (row g registered to
 * kept annotation g, smap_register_gt); counts: [B] int32 = smap_register_gt's matched_counts (clamped to 0..G); gt_2d: [B,G,15,4] f64 =
 * columns 0:4 (x, y, Z, score) of the kept annotations, 1 <= G <= SMAP_EVAL_MAXG; terms: scratch [B,G,SMAP_EVALMAPS_ACC_DOUBLES] f64.
 * Rows >= counts[b] are not read.  2D part: for a row whose predicted root has x > 0 and y > 0, every joint with gt score > 1 counts in
 * count_gt, and in count_pred / distance_e (+= dis / head) when dis = |gt - pred| < head = |gt head - gt neck| / 3, strictly.  Bone part:
 * for every sampled limb k (bone_mask), real = gt Z[dst] - gt Z[src]: distance_d += |depth_v - real|, count_pred_bone += 1,
 * reverse_count += 1 when depth_v * real < -1.  A frame's persons are summed into a zero partial first, the partial is then added to
 * acc -- the reference's association.  ONE launch of one workgroup while B * G <= 1024, two launches otherwise; same bits. */
int smap_evalmaps_update(const double* pred_2d, const double* depth_v, const int32_t* bone_mask, const int32_t* counts,
                         const double* gt_2d, int B, int G, double* terms, double* acc, void* stream);

/* ---- scoring MuPoTS-3D: lib/eval/mupots_smap.m and lib/eval/util_smap/ (3DPCK, AUC, MPJPE, ordinal rate) on the device ----
 * Joints in the protocol's order (head top, neck, right arm, left arm, right leg, left leg, pelvis); the predictions arrive in SMAP's
 * order (pose2d.mat / pose3d.mat) and are re-ordered where they are read.  F frames of S sequences, one after the other.
 *   gt2d [F,G,15,2], gt3d [F,G,15,3], occ [F,G,15] f64: annot2, univ_annot3 and occlusion_labels (first 15 columns) of every frame's
 *     VALID persons in annotation order; gt_count [F] int32 (clamped to 0..G), 1 <= G <= SMAP_MUPOTS_MAXG.
 *   pred2d [sumP,15,2] (pixels), pred3d [sumP,15,4] (mm; column 3 is not read) f64; frame f owns rows pred_offset[f] .. pred_offset[f + 1] - 1
 *     (int32 [F + 1]), at most SMAP_MUPOTS_MAXP of them; a range outside 0..sumP is read as no prediction.
 *   relative: both sides minus their pelvis; use_skel: the matched prediction's bones scaled to the ground truth's lengths;
 *     matched_only: EVALUATION_MODE 1, unmatched persons are not considered.
 * smap_mupots_frames, one wavefront per frame: the greedy matching (ground-truth persons in order; score = joints 2..14 within 40 px on
 * both axes, strictly, whose prediction is not at exactly (0, 0); the first prediction with the largest score > 0 wins and is not
 * offered again), then per (person, joint) the error sqrt(((dx*dx) + (dy*dy)) + (dz*dz)); an unmatched person's prediction is 100000
 * everywhere.  Rows out, written for g < gt_count[f] only: match [F,G] int32 (index inside the frame, -1 = unmatched), considered [F,G]
 * int32, err [F,G,15] f64, rootz [F,G,2] f64 = (the prediction's, the ground truth's) pelvis depth as the ordinal test reads them.
 * smap_mupots_fold, one thread per (sequence, field): acc [S, SMAP_MUPOTS_ACC_DOUBLES] f64 from the rows of frames seq_offset[s] ..
 * seq_offset[s + 1] - 1 (int32 [S + 1], clamped to 0..F), frames then persons in order; no atomics, every field is written.  Counts are
 * exact doubles.  Layout of a sequence's accumulator:
 *   0 considered persons | 1 annotated (valid) persons | 2 undetected (unmatched) persons | 3 ordinal pairs correct | 4 ordinal pairs
 *   (both 0 in relative mode) | 5 + 33 * j, j = 0..14: error sum, 31 counts of err < 0, 5, .. 150 (strict), count of err <= 150 |
 *   500 + 45 * m + 3 * j, m = 0 visible (1 - occ) / 1 occluded (occ): mask sum, sum of (NaN -> 160) * mask, count of that > 150.
 * float64 without contraction, correctly rounded square root and division (csrc/mupots_core.h is the text, for host and device). */
#define SMAP_MUPOTS_MAXG 16
#define SMAP_MUPOTS_MAXP 127
#define SMAP_MUPOTS_ACC_DOUBLES 590
int smap_mupots_frames(const double* gt2d, const double* gt3d, const int32_t* gt_count, const double* pred2d, const double* pred3d,
                       const int32_t* pred_offset, int F, int G, int sumP, int relative, int use_skel, int matched_only, int32_t* match,
                       int32_t* considered, double* err, double* rootz, void* stream);
int smap_mupots_fold(const int32_t* seq_offset, int S, const int32_t* gt_count, int F, int G, const int32_t* match,
                     const int32_t* considered, const double* err, const double* rootz, const double* occ, int relative, double* acc,
                     void* stream);

/* ---- label maps: dataset/representation.py generate_heatmap (:5-21) and generate_paf / putVecMaps3D (:36-113) on the device ----
 * labels: [B, S, SMAP_LABEL_C, H, W] fp32 out, the layout of JointDataset.__getitem__ (dataset/base_dataset.py:177-185): per label
 * scale 15 heat-maps (x 255), then per limb its x, y (x 127) and relative-depth channel.  Every value is written.
 * 8 <= H, 8 <= W, H * W <= 32768; 1 <= S <= SMAP_LABEL_MAX_SCALES; 1 <= P <= SMAP_LABEL_MAX_PERSONS; B * S <= 65535.
 * ksizes: HOST, [S][2] = (width, height) of every scale's blur kernel, as cv2.GaussianBlur takes them: odd, below SMAP_LABEL_MAX_TAPS.
 * table: DEVICE, 8-byte aligned, table_bytes long, what the host computed in float64 with the reference's own expressions
 * (smap_amd/labels.py pack_table); sections in this order, each starting on a multiple of 8 bytes, group = (b * S + s) * 14 + limb:
 *   limb_f   f64 [B*S*14][P][6]   per valid person of the group, IN ORDER: centerA_x, centerA_y (/ stride), unit_x, unit_y, limb_z, thre
 *   limb_box i32 [B*S*14][P][4]   min_x, max_x, min_y, max_y: the rounded box, half open, clipped to the map (:80-83)
 *   limb_n   i32 [B*S*14]         valid persons of the group (invalid or shorter than one cell: not in the table, :41-45,74-75)
 *   imp      i32 [B*15][P]        y * W + x of the distinct cells of joint j that hold an impulse (:10-14); other values are ignored
 *   imp_n    i32 [B*15]
 *   taps     f32 [S][2][SMAP_LABEL_MAX_TAPS]   the blur taps of every scale: [0] the row pass (along x), [1] the column pass
 * Counts outside 0..P are clamped.  Two launches on `stream`: one grid over (pixels, limb, frame x scale) for the fields, one workgroup
 * per (joint, frame x scale) for the heat-maps (blur, maximum, division).  DESIGN.md "Label maps" has the arithmetic. */
#define SMAP_LABEL_C 57                   /* 15 + 3 * 14 */
#define SMAP_LABEL_MAX_SCALES 8
#define SMAP_LABEL_MAX_TAPS 16
#define SMAP_LABEL_MAX_PERSONS 64
int smap_render_labels(const void* table, int64_t table_bytes, const int32_t* ksizes, int B, int S, int P, int H, int W, float* labels,
                       void* stream);

/* ---- training loss: SMAP._calculate_loss (model/smap.py:355-401) with JointsL2Loss / DepthLoss (lib/utils/loss_h.py), value and
 * gradient ----
 * heads: HOST array of 3 * n_heads DEVICE pointers, n_heads = 4 * stage_num, head h = 4 * stage + scale:
 *   heads[3 * h + 0] heatmap_2d [B, 43, H, W], heads[3 * h + 1] det_d [B, 14, H, W], heads[3 * h + 2] root_d [B, 1, H, W], fp32, dense.
 * labels [B, S, 57, H, W] fp32 as smap_render_labels writes them; head (stage i, scale j) is compared with label scale
 *   j + (i == stage_num - 1 && ctf).  2D channel c < 15 reads label channel c, c >= 15 reads 15 + 3 * ((c - 15) / 2) + (c - 15) % 2;
 *   det_d channel c reads 15 + 3 * c + 2.
 * valids [B, 57] fp32 in OUTPUT order (43 2D channels, then 14 det_d channels); a channel weighs 1 where valids > 0, else 0.
 * rdepth [B, R, 3] fp32 rows (y, x, Z); a row counts where Z > 0 and is read at cell (int(y), int(x)), truncated toward zero.
 * Per channel m = mean((out - label)^2) * weight, the difference in fp32, the sum in double in a fixed order (the same bits run to
 * run).  Per head: mean of m over (B, channels); with ohkm, on the finest head (j == 3) the `topk` largest of the 15 key-point channels
 * and the 2 * topk largest of the 28 PAF channels of every frame (mean + mean), and the topk largest of the 14 det_d channels; ties go
 * to the LOWER channel index.  Root: sum |root_d[cell] - Z| / count over the whole batch, 0 when no row counts.
 * total = sum over heads of (0.1 * 2D + 5 * depth + 10 * root), / 4 where j < 3.
 * result [8] fp32: total, 2D, bone, root (the three: finest heads summed over the stages), bad_rows, 0, 0, 0.  A counted row outside
 * [0, H) x [0, W) is never dereferenced; it is counted in bad_rows, and total is NaN then.
 * single != 0: ONE head (n_heads = 1, stage_num = 1, ctf = 0, label scale 0, S >= 1), treated as a finest head, all weights 1; any of
 *   its three tensors may be null and is left out then (labels / valids may be null when both maps are).
 * workspace: smap_loss_workspace_bytes(n_heads, B, R) bytes, 8-byte aligned; smap_loss_forward fills it (sums f64 [n_heads][B][57] at
 *   offset 0; csrc/loss_core.h workspace_layout has the rest) and smap_loss_backward reads it.
 * smap_loss_forward: two launches (reduce: one workgroup per (channel, frame, head); finish: one workgroup).
 * smap_loss_backward: one launch; upstream: DEVICE fp32 scalar, d L / d total.  grad: per head [B, 43, H, W] | [B, 14, H, W] |
 *   [B, 1, H, W], head after head (58 * B * H * W floats each); every element of a given tensor is written once,
 *   (out - label) * fp32(coef * upstream), root_d's from the root table.
 * 16-byte loads where H * W % 4 == 0 and every tensor is 16-byte aligned, 4-byte loads otherwise.
 * SMAP_E_ARG: null pointers, stage_num outside 1..4, S < 4 + ctf, topk outside 1..14 with ohkm, H * W outside 1..2^24, B or R outside
 * 1..65535, a workspace that is too small or misaligned.
 * smap_loss_finish_host: everything behind the reduction (csrc/loss_core.h, the text the device runs) on the HOST, all pointers
 * HOST: sums [n_heads][B][57], rd_at_rows [n_heads][B][R] = root_d at the rows' cells (anything for rows that do not count); out:
 * result [8], m / sel / coef [n_heads][B][57] (the per-channel loss, the 0 / 1 selection, the gradient factor),
 * root_cell [n_heads][B][R] (y * W + x, -1 for a row that does not count, -2 for one outside the map), root_fac [n_heads][B][R]
 * (10 * head factor * sign(out - Z) / count), part [n_heads][B][6] (per frame the sums of the kept m of the key-point | 2D, PAF and
 * depth groups, then of its rows: sum |root_d - Z|, rows counted, rows outside).
 * Needs no GPU. */
int64_t smap_loss_workspace_bytes(int n_heads, int B, int R);
int smap_loss_forward(const void* const* heads, const float* labels, const float* valids, const float* rdepth, int stage_num, int ohkm,
                      int topk, int ctf, int single, int B, int S, int R, int H, int W, void* workspace, int64_t workspace_bytes,
                      float* result, void* stream);
int smap_loss_backward(const void* const* heads, const float* labels, int stage_num, int ohkm, int topk, int ctf, int single, int B, int S,
                       int R, int H, int W, const void* workspace, int64_t workspace_bytes, const float* upstream, float* grad,
                       void* stream);
int smap_loss_finish_host(const double* sums, const float* valids, const float* rdepth, const float* rd_at_rows, int stage_num, int ohkm,
                          int topk, int ctf, int single, int B, int R, int H, int W, double* result, double* m, double* sel, double* coef,
                          int32_t* root_cell, double* root_fac, double* part);

/* ---- the same loss, forward only, from the heads WHERE THE ENGINE LEAVES THEM (validation loss: SMAP.forward with labels) ----
 * An all-heads schedule (smap_amd/engine.py Graph(all_heads=True)) keeps the 36 head tensors at their units' own resolutions; the
 * reference upsamples each to H x W (bilinear, align_corners) before it compares it with the labels.  smap_loss_forward_src does that
 * interpolation inside the reduction: no upsampled map is written or read back.
 * sources: HOST array of 3 * n_heads descriptors (n_heads = 4 * stage_num, no single-head mode), [3 * h + 0 / 1 / 2] = heatmap_2d (c = 43),
 *   det_d (c = 14), root_d (c = 1) of head h.  Element (frame b, pixel y, x, channel ch) of a source is the fp32 number at
 *   ptr[b * frame_stride + (y * w + x) * pix_stride + ch * ch_stride] (strides in floats): NHWC with a padded pixel
 *   (ch_stride = 1, pix_stride >= c) or NCHW (pix_stride = 1, ch_stride >= h * w).  h <= H and w <= W; a source of height or width 1 is
 *   legal, all its taps are index 0; a source of H x W is read as it is.  Frames 0 .. B - 1 are read, whatever lies behind them.
 * Value at an output pixel: ATen's align-corners index rule in fp32 and l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11),
 *   every operation rounded once -- the expression of the engine's head sum.  root_d is read the same way at the rows' cells.
 * Everything else (labels, valids, rdepth, the integers, result) as smap_loss_forward.  The workspace begins with smap_loss_forward's
 *   layout (sums, ..., rd_at, root_cell: what the shared finish launch reads and writes) followed by the per-chunk partial sums
 *   f64 [n_heads][B][ceil(H * W / 256)][57]; smap_loss_src_workspace_bytes has its size.  It does not feed smap_loss_backward; smap_loss_backward_src (below) is its gradient.
 * Three launches on `stream` (reduce: one workgroup per (256 output pixels, frame, head) over all 57 channels; fold: the chunks in
 *   order; finish), no atomics: the same bits run to run, and a frame's sums depend on that frame only.  No allocation, no
 *   synchronisation.
 * SMAP_E_ARG: as smap_loss_forward, and: a null or misaligned source pointer, c other than 43 / 14 / 1, a size below 1 or above H x W,
 *   strides that are neither of the two orders. */
struct smap_head_src {
    const float* ptr;
    int32_t h, w, c;
    int32_t pix_stride, ch_stride;
    int32_t reserved;
    int64_t frame_stride;
};
int smap_sizeof_head_src(void);
int64_t smap_loss_src_workspace_bytes(int n_heads, int B, int R, int H, int W);
int smap_loss_forward_src(const struct smap_head_src* sources, const float* labels, const float* valids, const float* rdepth, int stage_num,
                          int ohkm, int topk, int ctf, int B, int S, int R, int H, int W, void* workspace, int64_t workspace_bytes,
                          float* result, void* stream);

/* ---- the gradient of total at the heads' OWN resolution: the adjoint of smap_loss_forward_src's upsampling ----
 * Runs behind smap_loss_forward_src on the same sources, labels and integers, with the workspace as that call left it (read-only
 * here: coef, root_cell and root_fac of the leading smap_loss_forward layout; nothing behind it is needed).
 * grads: HOST array of 3 * n_heads descriptors, [i] = where the gradient of sources[i] goes: the same h, w, c, its own pointer and
 *   strides in either order (NCHW, or NHWC with a padded pixel).  A null ptr: that gradient is not wanted (the rest of the descriptor
 *   is not read).  Every one of the B x c x h x w described elements is written exactly once; padding floats and every other byte stay.
 * Value at source cell (i, j) of a 2D / depth channel: with up_p and the taps i0, i1, l0, l1 of smap_loss_forward_src at output pixel
 *   p = (y, x) and e_p = (up_p - label_p) * f, f = fp32(coef * upstream[0]):   sum_y wy(y, i) * sum_x wx(x, j) * e[y, x],
 *   wy(y, i) = l0(y) where i0(y) == i, plus l1(y) where i1(y) == i (both at the last source row), wx alike.  A source of H x W: e itself;
 *   one of height or width 1: the plain sum over that dimension.  f == 0: zeros, the channel's source and label planes are not read.
 *   root_d: zeros, then per counted row on the map, in row order, root_fac * upstream times the four tap weights of the row's cell.
 * Two launches on `stream`, no atomics, no allocation, no synchronisation.  part: one thread per (interval between source cells,
 *   channel, frame, head) reads its output pixels once -- every label element is read by exactly one thread -- and writes four partial
 *   sums (a pixel's first / second tap in y times first / second tap in x) to scratch; sources of H x W and root_d are finished there.
 *   fold: one thread per source cell adds the up to nine partial sums that name it in a fixed order.  The order of every sum depends on
 *   (h, w, H, W) alone: the same bits run to run and whichever of the two layouts sources and grads have.
 * scratch: 16-byte aligned, f32 [B][c][h][w][4] for each heatmap_2d / det_d tensor that is smaller than H x W and whose gradient is
 *   wanted.  smap_loss_backward_src_scratch_bytes (HOST, needs no GPU) sums that over all 2 * n_heads tensors of `sources` -- it knows
 *   neither H x W nor grads, so it is an upper bound; the call itself takes any buffer that holds what it needs.
 * upstream: DEVICE fp32 scalar, d L / d total.
 * SMAP_E_ARG: everything smap_loss_forward_src refuses (valids, rdepth and result are not taken), a grads[i] with a pointer whose h, w, c
 *   differ from sources[i]'s, whose pointer is misaligned or whose strides are neither order, a scratch buffer that is too small or
 *   misaligned, a null upstream. */
int64_t smap_loss_backward_src_scratch_bytes(const struct smap_head_src* sources, int n_heads, int B);
int smap_loss_backward_src(const struct smap_head_src* sources, const struct smap_head_src* grads, const float* labels, int stage_num,
                           int ohkm, int topk, int ctf, int B, int S, int R, int H, int W, const void* workspace, int64_t workspace_bytes,
                           void* scratch, int64_t scratch_bytes, const float* upstream, void* stream);

/* ---- the three head arms of one Upsample_unit, BN folded, in fp32: forward and its exact gradient (csrc/heads.hip) ----
 * One unit: P = B * h * w pixels, X = the unit's `out` [P, chl], arms a = 0, 1, 2 with C_a channels (43 | 14 | 1 in the network).
 *   forward   Z_a = X W1_a^T + b1_a      M_a = relu(Z_a)      Y_a = conv3x3(M_a, W2_a, pad 1) + b2_a
 *   backward  gb2_a = sum_p G_a          gW2_a[c, ci, t] = sum_p G_a[p, c] M_a[p + t, ci]   (p + t inside the image)
 *             gM_a = conv3x3^T(G_a, W2_a)   gZ_a = gM_a where Z_a > 0, else 0   gb1_a = sum_p gZ_a   gW1_a = gZ_a^T X   gX = sum_a gZ_a W1_a
 * x: X in one of three layouts, NHWC with frames back to back (frame stride h * w * pix_stride), pix_stride in ELEMENTS and a multiple
 *   of 4: SMAP_HEADS_X_F32 fp32, pix_stride >= chl, 16-byte aligned; SMAP_HEADS_X_F16 fp16, pix_stride >= chl, 8-byte aligned;
 *   SMAP_HEADS_X_F16_HILO fp16 [2][chl] per pixel (the engine's x3 planes), pix_stride >= 2 * chl, value = fp32(hi) + fp32(lo).
 * w1cat [3 * chl][chl], b1cat [3 * chl]: the three arms' folded 1x1 weights one after the other; w2 / b2: HOST arrays of three DEVICE
 *   pointers, w2[a] [C_a][chl][3][3], b2[a] [C_a]; all dense fp32 as torch keeps them.  gw1cat, gb1cat, gw2[a], gb2[a]: the same shapes.
 * y / g: HOST arrays of three smap_head_src, Y_a (written) and G_a (read): h x w, c = C_a in 1..64, NHWC with a padded pixel or NCHW.
 *   Every one of the B * C_a * h * w described elements of Y_a is written exactly once; padding floats and every other byte stay.
 * gx: fp32 NHWC [P] pixels of gx_pix_stride >= chl floats, chl written per pixel; null: not wanted, that launch is left out.
 * workspace: 256-byte aligned, smap_heads_ws_bytes(B, h, w, chl, backward) bytes (HOST, needs no GPU), floats, every region a multiple
 *   of 64 floats: M [P][3 * chl] (all the forward pass needs) | gZ [P][3 * chl] | part [slices][chl * max(3 * chl, 576)] |
 *   colpart [slices][3 * chl], slices = ceil(P / L), L = 256 pixels while P <= 16384, else ceil(P / 64) rounded up to 16.
 *   smap_heads_backward computes M again itself (it needs no earlier forward call) and leaves M and gZ there.
 * Arithmetic: every sum is an fp32 fmaf chain from 0 in a fixed order -- Z over ci; Y and gM over (chunk of 16 channels, tap, channel); gX over
 *   the 3 * chl columns of gZ; the pixel sums over the pixels of a slice in order, then the slices in order -- then the bias added
 *   once.  No atomics: the same bits run to run, and the same bits whichever layout holds the same values.
 * Launches on `stream`: forward 4, backward 12 (13 with gx).  No allocation, no synchronisation.
 * SMAP_E_ARG: null pointers, B outside 1..65535, h * w outside 1..2^24, P above 2^26, chl outside 64..1024 or not a multiple of 64,
 *   a stride smaller than its channels, an unknown layout, a misaligned pointer, a head descriptor of another size or with strides of
 *   neither order, a workspace that is too small or misaligned. */
#define SMAP_HEADS_X_F32 0
#define SMAP_HEADS_X_F16 1
#define SMAP_HEADS_X_F16_HILO 2
struct smap_heads_x {
    const void* ptr;
    int32_t layout;
    int32_t pix_stride;
};
int smap_sizeof_heads_x(void);
int64_t smap_heads_ws_bytes(int B, int h, int w, int chl, int backward);
int smap_heads_forward(const struct smap_heads_x* x, const float* w1cat, const float* b1cat, const float* const* w2, const float* const* b2,
                       const struct smap_head_src* y, int B, int h, int w, int chl, void* workspace, int64_t workspace_bytes, void* stream);
int smap_heads_backward(const struct smap_heads_x* x, const float* w1cat, const float* b1cat, const float* const* w2,
                        const struct smap_head_src* g, int B, int h, int w, int chl, float* gw1cat, float* gb1cat, float* const* gw2,
                        float* const* gb2, float* gx, int gx_pix_stride, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the trunk of one Upsample_unit, BN folded, in fp32: forward and its exact gradient (csrc/trunk.hip) ----
 * out = relu(u_skip(x) + up_conv(interpolate(out_prev))) (model/smap.py Upsample_unit.forward).  P = B * h * w pixels, X [P, cin];
 * O_prev [P', chl] at hp x wp, P' = B * hp * wp; I = bilinear align_corners interpolation hp x wp -> h x w by ATen's fp32 index and weight
 * rule.  The rows of I sum to 1, so the 1x1 is applied at LOW resolution and the result interpolated:
 *   forward   S = X Wu^T        U = O_prev Wc^T       O = relu((S + I(U)) + b),  b = bu + bc
 *   backward  gPre = gO where O > 0, else 0       gb = sum_p gPre  (the gradient of bu and of bc alike)
 *             gWu = gPre^T X    gX = gPre Wu      gU = I^T gPre [P', chl]      gWc = gU^T O_prev      gO_prev = gU Wc
 * x, o_prev: smap_heads_x descriptors (above) of h x w pixels of cin channels and of hp x wp pixels of chl channels, any of the three
 *   layouts.  o_prev null: the coarsest unit, no up path -- then hp and wp are 0 and wc, gwc and g_o_prev are null; otherwise none of them is.
 * wu [chl][cin], wc [chl][chl], b [chl]: dense fp32 as torch keeps them; gwu, gwc, gb: the same shapes.  b is 16-byte aligned.
 * o (written by forward, read by backward), g_o: dense fp32 [P][chl], 16-byte aligned.  g_o_prev: dense fp32 [P'][chl], written.
 * gx: fp32 NHWC [P] pixels of gx_pix_stride >= cin floats, cin written per pixel; null: not wanted, that launch is left out.
 * workspace: 256-byte aligned, smap_trunk_ws_bytes(B, h, w, hp, wp, cin, chl, backward) bytes (HOST, needs no GPU), floats, every region a
 *   multiple of 64 floats.  forward: S [P][chl] | U [P'][chl].  backward: gPre [P][chl] | gU [P'][chl] |
 *   part [max(slices * chl * cin, slices' * chl * chl)] | colpart [max(slices, slices')][chl] | colsum [chl], slices = ceil(P / L) by the
 *   slice rule of the heads block, slices' the same of P'.  The backward call needs no earlier forward call: it reads o.
 * Arithmetic: S, U, gX, gO_prev are fp32 fmaf chains from 0 over the input channels in order; gWu, gWc and gb over the pixels of a slice in
 *   order, then the slices in order; the interpolation is ATen's tap expression ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11); gU is
 *   an fmaf chain from 0 of (wy * wx) * gPre over the pixels whose taps name the cell, (y, x) ascending.  No atomics: the same bits
 *   run to run, and the same bits whichever layout holds the same values.
 * Launches on `stream`: forward 3 (1 without an up path); backward 3 without an up path, 8 with one, + 1 with gx.  No allocation, no
 *   synchronisation.
 * SMAP_E_ARG, before any HIP call: null pointers, B outside 1..65535, h * w or hp * wp outside 1..2^24, P or P' above 2^26, chl outside
 *   64..1024 or cin outside 64..4096 or either not a multiple of 64, an up path given in part (o_prev, wc, gwc, g_o_prev, hp, wp), a
 *   stride smaller than its channels, an unknown layout, a misaligned pointer, a workspace that is too small or misaligned. */
int64_t smap_trunk_ws_bytes(int B, int h, int w, int hp, int wp, int cin, int chl, int backward);
int smap_trunk_forward(const struct smap_heads_x* x, const struct smap_heads_x* o_prev, const float* wu, const float* wc, const float* b,
                       float* o, int B, int h, int w, int hp, int wp, int cin, int chl, void* workspace, int64_t workspace_bytes, void* stream);
int smap_trunk_backward(const struct smap_heads_x* x, const struct smap_heads_x* o_prev, const float* o, const float* wu, const float* wc,
                        const float* g_o, float* gwu, float* gwc, float* gb, float* g_o_prev, float* gx, int gx_pix_stride, int B, int h,
                        int w, int hp, int wp, int cin, int chl, void* workspace, int64_t workspace_bytes, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SMAP_HIP_H */
