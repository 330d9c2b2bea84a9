/*
 * arseg_hip.h -- C ABI of libarseg_hip.so: the MI355X (gfx950) kernels of AR-Seg's LR-branch
 * inference hot path.  This is the drop-in boundary: plain pointers and
 * sizes, no torch / C++ types.  Each entry point cites the reference interface it replaces
 * (paths relative to the AR-Seg repository).
 *
 * Conventions
 *   - All data pointers are DEVICE pointers unless the name ends in `_host`.
 *   - The caller owns every buffer (inputs, outputs, workspace).  Nothing is allocated here.
 *   - Every function only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and never synchronises the device.
 *   - Return value: 0 = ok; < 0 = ARSEG_E* (argument / shape problem, nothing was launched);
 *     > 0 = a hipError_t from the launch.  Nothing throws or aborts.
 *   - "NHWC" tensors are [N][H][W][ld] floats with `ld >= C` the per-pixel channel stride, so a
 *     channel slice of a wider tensor can be read or written in place (concat without copies).
 *   - No hidden global state; the library is thread-compatible (one stream per caller thread).
 *   - Non-finite values.  A NaN or an infinity in a float input reaches the output as it does in the torch expression an entry point
 *     restates (tests/test_gpu_nonfinite.py): (a) every output that depends on the element with non-zero weight is non-finite; (b) every
 *     output the fp64 reference keeps finite is finite and within the entry point's tolerance; (c) a NaN stays a NaN, and for the convs
 *     (every plan), scale_add, the pools, the global mean / max and the heads the non-finite outputs under a NaN are exactly the
 *     reference's.  The activations (ReLU / PReLU / none), the max pools, the global max, the nearest resize and the casts are selects,
 *     not v_max: NaN, +Inf and -Inf come out as torch's (ReLU: NaN -> NaN, -Inf -> 0).  Two kernels compute in tiles wider than an
 *     output's receptive field, and what they may make non-finite is the reference's set grown to whole tiles: Winograd F(4,3) (4 x 4
 *     output tiles on the dilation lattice: the 6 x 6 input transform mixes the tile) and the matrix-core CReFF kernels (2-row x 8-column
 *     query patches: P.V runs over all keys under a patch, with probability 0 outside a query's own window).  In ARSEG_MATH_F16X3 and in
 *     16-bit storage an infinity may come out as NaN (hi = Inf, lo = Inf - Inf): (a)-(c) hold, the Inf / NaN class is not kept.  A warp
 *     tap outside the image reads zeros (never a clamped pixel times weight 0): grid_sample(padding_mode='zeros').
 */
#ifndef ARSEG_HIP_H
#define ARSEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARSEG_ABI_VERSION 5

enum arseg_status {
    ARSEG_OK = 0,
    ARSEG_EINVAL = -1,        /* null pointer, non-positive size, misaligned pointer / stride */
    ARSEG_EUNSUPPORTED = -2,  /* shape outside what the kernels are built for (see each function) */
    ARSEG_EWORKSPACE = -3     /* workspace too small; query the *_workspace_bytes function */
};

enum arseg_act { ARSEG_ACT_NONE = 0, ARSEG_ACT_RELU = 1, ARSEG_ACT_PRELU = 2, ARSEG_ACT_SIGMOID = 3 };
enum arseg_layout { ARSEG_NCHW = 0, ARSEG_NHWC = 1, ARSEG_C8 = 2 /* [N][C/8][H][W][8], the CReFF kernel's layout */ };
enum arseg_flow_dtype { ARSEG_FLOW_F32 = 0, ARSEG_FLOW_F64 = 1 };
enum arseg_resize_mode { ARSEG_NEAREST = 0, ARSEG_BILINEAR = 1 };
enum arseg_reduce_op { ARSEG_REDUCE_MEAN = 0, ARSEG_REDUCE_MAX = 1 };
enum arseg_dtype { ARSEG_DT_F32 = 0, ARSEG_DT_F16 = 1, ARSEG_DT_BF16 = 2 };   /* storage element type of the 16-bit entry points */
enum arseg_creff_warp_impl { ARSEG_CREFF_WARP_AUTO = 0, ARSEG_CREFF_WARP_TILES = 1 /* creff_rr.hip */, ARSEG_CREFF_WARP_ROLL = 2 /* creff_roll.hip */ };
enum arseg_creff_impl { ARSEG_CREFF_AUTO = 0, ARSEG_CREFF_MFMA = 1 /* split-fp16 matrix-core kernel */, ARSEG_CREFF_VALU = 2 /* fp32 VALU kernel */ };

typedef void *arseg_stream_t; /* hipStream_t */

int arseg_version(void);
const char *arseg_status_string(int status);

/* ---------------------------------------------------------------------------------------------
 * The `localAttention` pair (third-party CUDA extension the reference imports at
 * model/attention.py:7-11; call sites model/attention.py:18 and :38).
 *   similar  : s[n,y,x,dy*kW+dx] = sum_c q[n,c,y,x] * k[n,c,y+dy-kH/2,x+dx-kW/2]   (0 outside)
 *   weighting: o[n,c,y,x]        = sum_i v[n,c,y+dy_i-kH/2,x+dx_i-kW/2] * w[n,y,x,i] (0 outside)
 * q,k,v,o: NCHW contiguous fp32; s,w: [N,H,W,kH*kW].  kH,kW odd, kH*kW <= 121.
 * ------------------------------------------------------------------------------------------- */
int arseg_local_similar_fwd(const float *q, const float *k, float *s, int N, int C, int H, int W, int kH, int kW,
                            arseg_stream_t stream);
int arseg_local_weighting_fwd(const float *v, const float *w, float *o, int N, int C, int H, int W, int kH, int kW,
                              arseg_stream_t stream);
/* The same pair on NHWC (torch.channels_last) features: element (n,c,y,x) at ((n*H + y)*W + x)*ld + c, ld >= C shared by the two inputs
 * (similar) / by v and o (weighting); s, w keep [N,H,W,kH*kW].  No layout change between the NHWC backbone tensors and the op. */
int arseg_local_similar_nhwc_fwd(const float *q, const float *k, int ld, float *s, int N, int C, int H, int W, int kH, int kW,
                                 arseg_stream_t stream);
int arseg_local_weighting_nhwc_fwd(const float *v, const float *w, int ld, float *o, int N, int C, int H, int W, int kH, int kW,
                                   arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * warpFeature(feature, flow)                                            evaluation.py:61-87
 * feature: [N,C,H,W] in `layout` (NCHW or NHWC with ld == C); out: same layout, or C8 when
 * out_layout == ARSEG_C8 (NHWC input only); flow: [N,H,W,2] (dx,dy) in feature pixels, fp32 or fp64.  Sampling = grid_sample(bilinear, zeros, align_corners=False) of the grid
 * normalised with 2*g/(W-1)-1, reproduced operation by operation (fp64 grid -> fp32 cast).
 * NHWC requires C % 4 == 0.
 * ------------------------------------------------------------------------------------------- */
int arseg_warp_fwd(const float *feature, const void *flow, int flow_dtype, float *out, int N, int C, int H, int W,
                   int layout, int out_layout, arseg_stream_t stream);

/* Motion-vector resize block                                            evaluation.py:176-180
 * mv_q: int16 quarter-pel [N,H,W,2] exactly as stored on disk (dataset/camvid.py:624-626,
 * dataset/cityscapes.py:282-285); out: fp64 [N,Hp,Wp,2] = bilinear(align_corners=True) of
 * (mv_q/4) * Hp/H (both components scaled by Hp/H as the reference does). */
int arseg_mv_resize_fwd(const int16_t *mv_q, double *out, int N, int H, int W, int Hp, int Wp, arseg_stream_t stream);

/* The same block for a float flow field [N,H,W,2] in pixels (fp32 or fp64; the reference's DataLoader hands over fp64 = int16/4):
 * out fp64 [N,Hp,Wp,2] = bilinear(align_corners=True) of flow * Hp/H, computed in fp64. */
int arseg_flow_resize_fwd(const void *flow, int flow_dtype, double *out, int N, int H, int W, int Hp, int Wp, arseg_stream_t stream);

/* The two steps above fused (fast path): warp an NHWC feature straight from the int16 MV map;
 * out_layout = ARSEG_NHWC or ARSEG_C8. */
int arseg_warp_mvq_fwd(const float *feature, const int16_t *mv_q, float *out, int N, int C, int Hp, int Wp, int H,
                       int W, int out_layout, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * CReFF: MyAttention.forward(hr_feat, lr_feat) [+ final 1x1 classifier]
 *                                   model/attention.py:184-213; model/pspnet.py:219-231;
 *                                   model/bisenet.py:565-575
 * One fused kernel: bilinear(align_corners=True) upsample of lr, the three depthwise 3x3 convs
 * (+bias), the kH x kW local QK^T with zero-score padding taps, softmax over all kH*kW taps,
 * PV, residual add; optionally the 1x1 classifier (+ log-softmax over classes) on the result.
 *   hr   : C8 [N,C/8,Hp,Wp,8]  (already warped; arseg_warp*_fwd can write it directly)
 *   lr   : NHWC [N,hp,wp,C] (ld == C)
 *   wq/wk/wv : depthwise weights packed [9][C] (tap-major), bq/bk/bv : [C]
 *   p_out: C8 [N,C/8,Hp,Wp,8]   (channel-blocked so that the kernel's 8-channel chunks are contiguous)
 *   logits: NCHW [N,n_cls,Hp,Wp] or NULL (then wf/bf are ignored); wf: [n_cls][C], bf: [n_cls];
 *   log_softmax != 0 applies LogSoftmax over the class dimension (PSPNet head).
 * Supported: C % 8 == 0, kH == kW in {3,5,7}, n_cls <= 32, N*C*Hp*Wp*4 < 2 GiB.
 * ------------------------------------------------------------------------------------------- */
int arseg_creff_fwd(const float *hr, const float *lr, const float *wq, const float *bq, const float *wk,
                    const float *bk, const float *wv, const float *bv, float *p_out, const float *wf, const float *bf,
                    int n_cls, float *logits, int log_softmax, int N, int C, int Hp, int Wp, int hp, int wp, int kH,
                    int kW, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * warpFeature + MyAttention.forward + final 1x1 classifier in ONE kernel (the non-keyframe tail of
 * EvalAlterRes, evaluation.py:176-193, for the 64-channel full-resolution PSPNet feature):
 *                                   evaluation.py:61-87,176-180; model/attention.py:184-213;
 *                                   model/pspnet.py:219-231
 * The keyframe feature is read UN-warped and sampled with the frame's motion vectors while a tile
 * is staged, so the warped tensor never exists in memory.
 *   ref_nhwc_host : HOST array of N device pointers; entry i = keyframe feature of frame i,
 *                   NHWC [Hp][Wp][C] (ld == C).  Frames of one GOP pass the same pointer.
 *   mv_q : int16 quarter-pel [N,H,W,2] as in arseg_warp_mvq_fwd (resized to (Hp,Wp) in fp64 in-kernel)
 *   lr, wq..bv, wf, bf, logits, log_softmax : as arseg_creff_fwd
 *   p_out : the fused feature, layout p_layout = ARSEG_C8 [N,C/8,Hp,Wp,8] or ARSEG_NHWC [N,Hp,Wp,C]
 * Supported: C == 64, kH == kW == 7, N <= 32, n_cls <= 32, C*Hp*Wp*4 < 2 GiB per frame (the rolling
 * kernel addresses every frame through its own buffer descriptor; launches that fall to the tile kernel --
 * 17-32 classes, impl = TILES -- need N*C*Hp*Wp*4 < 2 GiB); anything else returns ARSEG_EUNSUPPORTED and the
 * caller uses arseg_warp_mvq_fwd + arseg_creff_fwd or splits the batch.
 * ------------------------------------------------------------------------------------------- */
int arseg_creff_warp_fwd(const float *const *ref_nhwc_host, const int16_t *mv_q, int H, int W, const float *lr,
                         const float *wq, const float *bq, const float *wk, const float *bk, const float *wv,
                         const float *bv, float *p_out, int p_layout, const float *wf, const float *bf, int n_cls,
                         float *logits, int log_softmax, int N, int C, int Hp, int Wp, int hp, int wp, int kH, int kW,
                         arseg_stream_t stream);

/* The same with the kernel choice made explicit (measurements, tests): impl = enum arseg_creff_warp_impl -- AUTO / ROLL: the rolling
 * kernel (creff_roll.hip: a workgroup walks down a 16-column strip, key / value records of the 7 x 7 windows in LDS rings, producer and
 * consumer waves of different rows overlap); TILES: the 16 x 16 tile kernel of rounds 2-3 (creff_rr.hip).  seg_rows = rows of a strip
 * segment (> 0: the rolling kernel works on fixed segments of that many rows, rounded up to even, and raised if a workgroup would get more
 * than 64 of them; 0 = default: whole strips dealt to the workgroups, the remainder cut into equal runs of row pairs); max_wgs = upper bound on its persistent
 * workgroups (0 = one per compute unit; fewer leave compute units to kernels of other streams).  No environment variables are read.
 * Both kernels compute in split fp16: the operand range stated at arseg_creff_fwd_ex (full precision for |Q|, |K|, |V|, |p_out| <= 65504,
 * 11-bit lo halves up to 131008, a silent clamp beyond, an absolute floor of 2^-24 for small features, no range watch) holds for them as it
 * stands, the warped keyframe feature taking the place of hr; tests/test_gpu_creff_accuracy.py holds every schedule of both to it. */
int arseg_creff_warp_fwd_ex(const float *const *ref_nhwc_host, const int16_t *mv_q, int H, int W, const float *lr,
                            const float *wq, const float *bq, const float *wk, const float *bk, const float *wv,
                            const float *bv, float *p_out, int p_layout, const float *wf, const float *bf, int n_cls,
                            float *logits, int log_softmax, int N, int C, int Hp, int Wp, int hp, int wp, int kH, int kW,
                            int impl, int seg_rows, int max_wgs, arseg_stream_t stream);

/* Which kernel arseg_creff_warp_fwd_ex runs for a launch of this shape and these knobs -- a pure query, nothing is launched: returns
 * ARSEG_CREFF_WARP_ROLL or ARSEG_CREFF_WARP_TILES (> 0), ARSEG_EUNSUPPORTED for shapes the fused entry point does not cover (or impl = ROLL on a
 * launch the rolling kernel does not admit), ARSEG_EINVAL for bad arguments.  n_cls = 0: no head.  The rule: the rolling kernel serves every
 * launch it admits (C == 64, 7 x 7, no head or <= 16 classes, a schedule that fits its 64-entry piece table); the tile kernel serves 17-32-class
 * heads, oversized schedules and impl = TILES.  (bench.py labels its roofline line with this; tests enforce the table.) */
int arseg_creff_warp_select(int N, int C, int Hp, int Wp, int hp, int wp, int kH, int kW, int n_cls, int impl, int seg_rows, int max_wgs);

/* The rolling kernel on 16-bit features: the keyframe features (ref_nhwc_host: HOST array of N device pointers, NHWC [Hp][Wp][C]) and lr
 * ([N,hp,wp,C]) are fp16 or bf16 (dtype = ARSEG_DT_F16 | ARSEG_DT_BF16, both the same) and are read as they are -- no fp32 copies; every
 * element is widened to fp32 in registers (exact) and everything behind the loads is the arithmetic of arseg_creff_warp_fwd_ex, so the
 * results equal, bit for bit, those of arseg_creff_warp_fwd_ex on the same tensors cast to fp32.  Weights, biases, the classifier, p_out and
 * logits are fp32; every other argument as arseg_creff_warp_fwd_ex.  It serves exactly the launches for which
 * arseg_creff_warp_select(..., impl = ARSEG_CREFF_WARP_ROLL, ...) answers ARSEG_CREFF_WARP_ROLL; anything else (C != 64, other windows, more than 16
 * classes, N > 32, a schedule beyond the piece table) returns ARSEG_EUNSUPPORTED before any launch -- the tile kernel has no 16-bit form
 * and nothing is computed in part; null pointers, another dtype or bad sizes ARSEG_EINVAL. */
int arseg_creff_warp16_fwd_ex(const void *const *ref_nhwc_host, const void *lr, int dtype, const int16_t *mv_q, int H, int W,
                              const float *wq, const float *bq, const float *wk, const float *bk, const float *wv,
                              const float *bv, float *p_out, int p_layout, const float *wf, const float *bf, int n_cls,
                              float *logits, int log_softmax, int N, int C, int Hp, int Wp, int hp, int wp, int kH, int kW,
                              int seg_rows, int max_wgs, arseg_stream_t stream);

/* The same with the kernel choice made explicit (measurements, tests): impl = enum arseg_creff_impl (AUTO: the matrix-core kernel
 * for C >= 128, the VALU kernel otherwise); mfma_tile_rows = 0 (by launch size), 8 or 16.  No environment variables are read.
 * Operand range of the matrix-core kernels (creff_mfma.hip behind this entry point; creff_roll.hip and creff_rr.hip behind
 * arseg_creff_warp_fwd_ex; the VALU kernel is plain fp32 and has none): fp32 emulated on the fp16 matrix cores.  Five operands are split
 * into hi + lo fp16 halves rounded toward zero (22 significant bits): the query, key and value conv results Q, K, V, the un-normalised
 * softmax weights P = exp(s - max) <= 1, and, for the classifier, the fused feature p_out and Wf.  A product is a_hi.b_hi + a_lo.b_lo +
 * a_hi.b_lo + a_lo.b_hi with fp32 accumulation, error ~2^-21 relative per operand, one-sided.  Full precision needs |x| <= 65504 for
 * every split operand; up to 131008 = 2 x 65504 the lo half keeps only 11 bits of x - 65504 (error up to 2^-11 of x); beyond, the pair
 * clamps to +-131008 -- silently: the conversion never produces an infinity from a finite value, and no NaN appears.  Below the fp16 normal
 * range a lo half is subnormal, an ABSOLUTE step of 2^-24 = 6e-8: uniformly small features (|V|, |p_out| << 1) carry an absolute error of
 * up to 2^-24 (1 + 49 max|V|) in p_out whatever their magnitude, e.g. 2e-5 relative at |V| ~ 4e-3.  Nothing is scaled (the conv engine
 * scales its weights per channel; Q, K, V here are split as computed) and there is NO range watch: unlike arseg_conv_desc.range_flag no
 * device word reports an operand outside the range, so a caller whose features may leave O(1e-2) .. 65504 pins impl = ARSEG_CREFF_VALU
 * (the fused entry point has no fp32 kernel: there, arseg_warp_mvq_fwd + this one).  Inside the range the result is within 4x (8x for
 * one saturated-softmax case, where the fp32 loop itself is a single rounding) the error of the plain fp32 loop against fp64, for p_out
 * and the logits; the statement, the clamp and the floor are tested for every kernel in tests/test_gpu_creff_accuracy.py (bounds and
 * their CPU proof: tests/creff_accuracy.py, tests/test_creff_accuracy.py). */
int arseg_creff_fwd_ex(const float *hr, const float *lr, const float *wq, const float *bq, const float *wk,
                       const float *bk, const float *wv, const float *bv, float *p_out, const float *wf, const float *bf,
                       int n_cls, float *logits, int log_softmax, int N, int C, int Hp, int Wp, int hp, int wp, int kH,
                       int kW, int impl, int mfma_tile_rows, arseg_stream_t stream);

/* Layout changes to / from C8 at the API boundary (layout = ARSEG_NCHW or ARSEG_NHWC; ld = NHWC channel stride). */
int arseg_to_c8_fwd(const float *in, int layout, int in_ld, float *out, int N, int C, int HW, arseg_stream_t stream);
int arseg_from_c8_fwd(const float *in, float *out, int layout, int out_ld, int N, int C, int HW, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * conv2d (+ folded BatchNorm / bias, + residual add, + activation) as an implicit GEMM on the
 * matrix cores: desc.math selects the back end -- ARSEG_MATH_F16X3 (default of the Python side: every fp32 operand split
 * into hi + lo fp16, three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation; operand range below) or ARSEG_MATH_F32
 * (v_mfma_f32_32x32x2_f32).  Replaces every nn.Conv2d/BatchNorm2d/ReLU/PReLU stack of
 * model/extractors.py:35-66,108-158, model/pspnet.py:14-46 and model/bisenet.py:31-60,162-399.
 *   out[n,oy,ox,co] = act( scale[co] * sum_{r,s,ci} in[n, oy*stride-pad+r*dil, ox*stride-pad+s*dil, ci]
 *                                        * w[co][(r*S+s)*Cin+ci]  + bias[co] + residual[n,oy,ox,co] )
 * in: NHWC (in_ld), Cin % 4 == 0 (pad RGB to 4), Cin a power of two unless R*S == 1.
 * w_packed: [Cout][Kpad] from arseg_pack_conv_weight_host.  scale/bias: [Cout] or NULL (1 / 0).
 * residual: NHWC (res_ld) or NULL.  tile_cfg / split_k: 0 = choose automatically.
 * ------------------------------------------------------------------------------------------- */
typedef struct arseg_conv_desc {
    int N, H, W, Cin, in_ld;
    int Cout, out_ld, res_ld;
    int R, S, stride, pad, dil;
    int act;           /* enum arseg_act */
    float prelu_slope; /* single shared slope (nn.PReLU() default, model/pspnet.py:40) */
    int tile_cfg;      /* 0 auto; 1..4 = 128x128, 128x64, 64x64, 64x128 (K step 32) with a double-buffered LDS tile; 5..8 = the
                          same tiles single-buffered (half the LDS, more workgroups per CU); 9..12 = single-buffered, K step 64;
                          13..16 = patch-resident kernel for 3x3 stride-1 pad==dil convs under ARSEG_MATH_F16X3 (Cin % 32 == 0): the
                          input patch of a 128- (13, 14) or 256-pixel (15, 16) tile stays in LDS for all nine taps, BN = 64 / 128;
                          ARSEG_EUNSUPPORTED for other shapes; 17..19 = 256x128, 128x256, 256x256 tiles on 8 / 16 waves (F16X3 only):
                          more MFMA work per byte fetched from L2 / Infinity Cache, for wide GEMMs that fill the chip; 20..22 (r6) = the
                          patch-resident kernel with BN = 64 on squarer pixel tiles (20: 256 pixels as 8 x 32, 21: 16 x 16, 22: 128 pixels as
                          8 x 16: less halo per output than the 4 x 64 / 2 x 64 tiles 13..16 take on a wide map); refused on narrower maps;
                          23 = the persistent kernel of arseg_conv_up2_c64_fwd (below): upsample2x, 3x3 stride 1 pad 1, Cin = Cout = 64,
                          F16X3, no residual, out_ld % 4 == 0, `out` 16-byte aligned; ARSEG_EUNSUPPORTED for anything else (ARSEG_EINVAL without
                          upsample2x: the id is defined for convs on an upsampled input only) */
    int split_k;       /* 0 auto, >= 1 explicit */
    /* batched mode (used by the Winograd path): `batch` independent problems of identical shape, problem b reads
       in + b*in_batch_stride, w_packed + b*w_batch_stride and writes out + b*out_batch_stride (strides in floats);
       batch <= 1 = a single problem.  No residual and no split-K in batched mode. */
    int batch;
    long long in_batch_stride, w_batch_stride, out_batch_stride;
    int math;          /* enum arseg_math: which MFMA back end evaluates the fp32 GEMM (selects the w_packed format too) */
    int upsample2x;    /* 1: `in` is the LOW-resolution tensor [N, H/2, W/2, in_ld] and the conv runs on its x2 bilinear
                          (align_corners=False) upsample, which is never materialised (PSPUpsample, model/pspnet.py:43-46): H, W stay
                          the conv's input size, both even, dil == 1.  Patch-resident plans only (tile_cfg 13..16 here; 5..8 and
                          10..13 of arseg_conv2d16_fwd, whose auto plan 0 is then 7); ARSEG_EUNSUPPORTED otherwise -- the Winograd
                          route has its own fused form (arseg_wino43_input_fwd upsample2x). */
    void *range_flag;  /* ARSEG_MATH_F16X3 only, may be NULL: a caller-owned, 4-byte aligned device word.  Bit 0 is set (atomic OR, never
                          cleared by the library) when an activation this conv multiplies exceeds range_limit in magnitude, i.e. when
                          the hi/lo fp16 pair starts to lose bits (65504) or clamps (131008): the caller reads the word once per
                          batch of launches and repeats the batch with ARSEG_MATH_F32 if it is set.  The Winograd route passes the
                          same word to its batched GEMM, which watches the TRANSFORMED activations it actually multiplies.  No host
                          synchronisation, one v_max3 per 2 activations in 1 / (Cout / tile) of the workgroups. */
    float range_limit; /* <= 0: 65504 */
} arseg_conv_desc;

/* ARSEG_MATH_F32:   v_mfma_f32_32x32x2_f32 on the fp32 operands; w_packed from arseg_pack_conv_weight_host.
 * ARSEG_MATH_F16X3: fp32 emulated on the fp16 matrix cores: x = hi + lo (two fp16, 22 significant bits),
 *                   a.b = a_hi.b_hi + a_hi.b_lo + a_lo.b_hi with fp32 accumulation (error ~2^-21 relative per product,
 *                   activations must satisfy |x| <= 131008 = 2 x 65504: the hi/lo pair clamps beyond, full 22-bit precision below 65504; |x| below the fp16 normal range carries an absolute error <= 6e-8).  w_packed from arseg_split_weight_f16x3_host, and `scale` must
 *                   carry that function's per-channel chan_mul_inv factor.  The bound is tested for every plan and route that computes
 *                   this way (every tile_cfg, split-K, the Winograd, LDS-DMA GEMM, tap and PSP routes): max|err| / max|out| against fp64
 *                   within 4x (8x on two K = 64 cases) the error of the plain fp32 loop (tests/test_gpu_split_accuracy.py).
 * ARSEG_MATH_F16:   reduced precision: plain fp16 operands (activations rounded to nearest, the hi halves of the same split
 *                   weights), one fp16 MFMA per product, fp32 accumulation; ~1e-3 relative error per conv.  Not used by default. */
enum arseg_math { ARSEG_MATH_F32 = 0, ARSEG_MATH_F16X3 = 1, ARSEG_MATH_F16 = 2 };

int arseg_conv_out_hw(const arseg_conv_desc *d, int *Ho, int *Wo);
size_t arseg_conv2d_workspace_bytes(const arseg_conv_desc *d);
int arseg_conv2d_fwd(const arseg_conv_desc *d, const float *in, const float *w_packed, const float *scale,
                     const float *bias, const float *residual, float *out, void *workspace, size_t workspace_bytes,
                     arseg_stream_t stream);

/* What a descriptor would launch, asked without a device: the verdict arseg_conv2d_fwd (engine = ARSEG_CONV_ENGINE_F32) or arseg_conv2d16_fwd
 * (ARSEG_CONV_ENGINE_16) gives before it looks at its pointers -- ARSEG_OK, ARSEG_EINVAL or ARSEG_EUNSUPPORTED -- and the plan behind it.  kind ..
 * split_k_allowed describe the id d->tile_cfg alone (the table of csrc/conv_plans.h; kind = ARSEG_PLAN_NONE for a number that is no id of the
 * engine) and are filled whatever the verdict, so a descriptor with nothing but tile_cfg set reads the table; on ARSEG_OK bm / bn / bk hold the
 * tile of this shape (the auto plans choose one) and the remaining fields are filled.  The 16-bit engine's bn is its channel tile, bk its K
 * step in halves, bm its pixel tile.  arseg_conv2d_workspace_bytes is workspace_bytes of the fp32 engine (0 on any other verdict). */
enum arseg_conv_engine { ARSEG_CONV_ENGINE_F32 = 0, ARSEG_CONV_ENGINE_16 = 1 };
enum arseg_conv_plan_kind { ARSEG_PLAN_NONE = 0, ARSEG_PLAN_AUTO, ARSEG_PLAN_TILE, ARSEG_PLAN_TILE_WIDE /* 8 / 16 waves */, ARSEG_PLAN_PATCH,
                            ARSEG_PLAN_STEM, ARSEG_PLAN_UP2_C64 };
typedef struct arseg_conv_plan_info {
    int kind;                            /* enum arseg_conv_plan_kind */
    int bm, bn, bk, nbuf;                /* tile: output pixels x output channels, K step, LDS stages (0: chosen per shape) */
    int fuses_upsample, split_k_allowed; /* the plan applies upsample2x itself | may take split-K */
    int nsplit;                          /* K slices of this launch */
    int patch_tw, patch_th;              /* patch-resident plans: the pixel tile (0 otherwise) */
    int Ho, Wo;
    size_t workspace_bytes;
} arseg_conv_plan_info;
int arseg_conv_plan_query(int engine, const arseg_conv_desc *d, arseg_conv_plan_info *info);

/* tile_cfg 23 of arseg_conv2d_fwd by itself: the 64 -> 64 channel 3x3 stride-1 pad-1 conv on the x2 bilinear upsample of `in`
 * (d->upsample2x = 1, ARSEG_MATH_F16X3; PSPNet's up_3) with the folded scale / bias / activation epilogue, no residual.  One persistent
 * workgroup per compute unit walks a run of 8 x 16 pixel tiles: four waves keep the layer's split weights in registers and multiply,
 * four stage the next tile's upsampled patch (csrc/conv_up2_c64.hip).  d->tile_cfg is ignored; no workspace.  max_wgs > 0 caps the
 * number of workgroups (0: one per compute unit, at most one per tile); results do not depend on it.  range_flag as in arseg_conv_desc. */
int arseg_conv_up2_c64_fwd(const arseg_conv_desc *d, const float *in, const float *w_packed, const float *scale, const float *bias,
                           float *out, int max_wgs, arseg_stream_t stream);

/* Plan selection ("find", what MIOpen calls miopenFindConvolutionForwardAlgorithm; the reference gets it implicitly from
 * torch.backends.cudnn.benchmark, train.py / evaluation.py): runs every launch plan the shape admits -- all tile_cfg it supports x
 * split-K {1,2,3,4,6,8}, plus the built-in heuristic (0,0) -- `reps` times each (<= 0: 3) on the caller's buffers, times them with
 * HIP events and returns the fastest as (*tile_cfg, *split_k) for arseg_conv_desc, its time in *best_us (may be NULL).
 * d->tile_cfg / d->split_k are ignored.  `workspace` should hold arseg_conv2d_find_workspace_bytes(d) bytes (candidates needing more
 * than workspace_bytes are skipped).  The ONLY entry point that synchronises the stream; `out` holds a valid result afterwards.
 * Returns the error of the heuristic plan if no candidate could be launched. */
size_t arseg_conv2d_find_workspace_bytes(const arseg_conv_desc *d);
int arseg_conv2d_find(const arseg_conv_desc *d, const float *in, const float *w_packed, const float *scale, const float *bias,
                      const float *residual, float *out, void *workspace, size_t workspace_bytes, int reps, int *tile_cfg,
                      int *split_k, float *best_us, arseg_stream_t stream);

/* Winograd F(4x4,3x3) path for 3x3 stride-1 convs with pad == dil (model/extractors.py:30-32 conv3x3, model/pspnet.py:38):
 *   V[36][T][Cin]  = arseg_wino43_input_fwd(in NHWC)          T = arseg_wino43_tiles(N,H,W,dil)
 *   M[36][T][Cout] = 36 GEMMs V[k] x U[k]^T                   arseg_conv2d_fwd in batched mode (batch = 36, 1x1)
 *   out NHWC       = arseg_wino43_output_fwd(M) with the usual scale / bias / residual / activation epilogue
 * U = arseg_wino43_pack_weight_host(w OIHW) -> [36][Cout][Cin] (Cin % 32 == 0 so that it is a valid packed 1x1 weight).
 * Operand range under ARSEG_MATH_F16X3: the GEMM operands are the TRANSFORMED activations V = B^T d B, up to 100x (typically ~10x) the
 * activations, so unscaled the split-fp16 range (|V| <= 131008) is reached for |x| >~ 1.3e3 in the worst case (beyond it V clamps): pass
 * v_scale = 2^-4 / m_scale = 2^4 (what the Python layer does) to move the limit to |x| ~ 2e4 worst case; the price is the absolute
 * floor of the low fp16 half (subnormal step 2^-24) rising to 2^-20 in units of V, still below Winograd's own fp32 rounding for O(1) data.
 * 2.25x..4x fewer MACs than the direct form; fp32 rounding error ~1e-5 relative instead of ~1e-6. */
long long arseg_wino43_tiles(int N, int H, int W, int dil);
/* upsample2x != 0: `in` is the low-resolution tensor [N,H/2,W/2,C] and the x2 bilinear (align_corners=False) upsample of
 * PSPUpsample (model/pspnet.py:45) is applied on the fly (H, W = upsampled size, even; dil == 1). */
/* v_scale / m_scale: V is stored multiplied by v_scale (> 0), M is multiplied by m_scale before the epilogue; with powers of two and
 * m_scale = 1 / v_scale the result is unchanged bit for bit while the GEMM operands shrink -- under ARSEG_MATH_F16X3 the transformed
 * activations (up to 100x, typically ~10x the input) otherwise leave the split-fp16 range for |x| >~ 1.3e3.  1.0f = no scaling. */
int arseg_wino43_input_fwd(const float *in, int in_ld, float *V, int N, int H, int W, int C, int dil, int upsample2x, float v_scale,
                           arseg_stream_t stream);
/* The same transform with V written in the split-row operand format of arseg_gemm_x3_fwd (C % 32 == 0, V_split 16-byte aligned, the
 * same T*C*4 bytes per frequency): the 36 GEMMs then run as ONE arseg_gemm_x3_fwd(V_split, U_f16x3, M, T, Cout, C, ..., batch = 36).
 * range_flag / range_limit: as in arseg_conv_desc -- the transform is where the fp32 operands of that GEMM are last seen. */
int arseg_wino43_input_split_fwd(const float *in, int in_ld, void *V_split, int N, int H, int W, int C, int dil, int upsample2x,
                                 float v_scale, void *range_flag, float range_limit, arseg_stream_t stream);
int arseg_wino43_output_fwd(const float *M, const float *scale, const float *bias, const float *residual, int res_ld, float *out,
                            int out_ld, int N, int H, int W, int Cout, int dil, int act, float prelu_slope, float m_scale,
                            arseg_stream_t stream);

/* The per-image pyramid operand of arseg_gemm_x3_cat_fwd for the folded PSP bottleneck (model/pspnet.py:14-31) in one pass:
 * out[n][co][k] (split rows, K = 64) = t[n][k][co] * unscale[co] for k < rows, 0 beyond.  t fp32 [N, rows, Cout], rows <= 64.
 * range_flag / range_limit: as in arseg_conv_desc -- this pass is where the fp32 values of that GEMM operand are last seen (un-scaled
 * pyramid terms can leave the split-fp16 range when the folded scale of a channel is small); NULL: no watch. */
int arseg_psp_w2_split_fwd(const float *t, const float *unscale, void *out, int N, int rows, int Cout, void *range_flag, float range_limit,
                           arseg_stream_t stream);

/* (Part of the nn.Conv2d replacement above: the GEMM inside conv3x3 on the Winograd route, /root/reference/model/extractors.py:30-32,
 * the 1x1 bottleneck of PSPModule, model/pspnet.py:26, and the low-resolution tap GEMM of PSPUpsample, model/pspnet.py:38-46.)
 * Batched GEMM on operands that are already split into fp16 (hi, lo) pairs ("split rows": a row of K values, K % 32 == 0, is K/32
 * groups of 128 bytes = 32 hi halves then 32 lo halves; the f16x3 weight format of arseg_split_weight_f16x3_host, now also for the
 * activations):   out[b][m][n] = act(scale[n] * sum_k x[b][m][k] * w[b][n][k] + bias[n] + residual[m][n])   (scale / bias / residual may
 * be NULL; residual fp32 [M][res_ld], batch == 1 only)
 * x_split [batch][M][K], w_split [batch][N][K] in split rows (batch strides in BYTES, multiples of 16), out fp32 [batch][M][out_ld]
 * (stride in floats), N % 4 == 0.  Operands reach LDS by LDS-DMA, no register staging (csrc/gemm_x3.hip).  tile_cfg 0..11
 * (M x N per workgroup): 0 = 256x256 with 8 waves, 1 = 256x256 with 16, 2 / 5 = 128x256 with 8 / 16, 3 = 128x128,
 * 4 = 256x128, 6 = 256x256 with 16 waves in two groups half a K step apart; 7 = 256x64, 8 = 128x64 with 4 waves, 9 = 128x64, 10 = 64x128, 11 = 128x128 with 32x64 wave
 * tiles (round 5: narrow tiles for 64- / 128-channel outputs; anything else: ARSEG_EINVAL).  out_split != 0: `out` is written as split rows too (N % 32 == 0, out_ld == N) -- it is the next GEMM's x_split, e.g. the
 * PSP bottleneck feeding the tap-decomposed up_1 conv.  The same fp32-grade arithmetic as ARSEG_MATH_F16X3 (three fp16 MFMAs per product).
 * arseg_split_rows_fwd converts fp32 rows [rows][in_ld] (times `mul`, a power of two keeps it exact) to split rows [rows][K].
 * range_flag / range_limit (may be NULL / <= 0: 65504): the operand range word of arseg_conv_desc, set by whoever WRITES split rows from
 * fp32 values (the split pass, a GEMM with out_split) -- the consuming GEMM never sees the fp32 operand. */
int arseg_split_rows_fwd(const float *in, long long in_ld, void *out_split, long long rows, int K, float mul, void *range_flag,
                         float range_limit, arseg_stream_t stream);
int arseg_gemm_x3_fwd(const void *x_split, const void *w_split, float *out, int M, int N, int K, int out_ld, int batch,
                      long long x_batch_stride, long long w_batch_stride, long long out_batch_stride, const float *scale,
                      const float *bias, const float *residual, int res_ld, int act, float prelu_slope, int out_split, int tile_cfg,
                      void *range_flag, float range_limit, arseg_stream_t stream);
/* The same GEMM over a K-concatenated operand pair: out = act(scale * (x . w^T + x2 . w2^T) + bias), x2 [batch][M][K2], w2 [batch][N][K2] split rows
 * with their own batch strides (0 = shared by the batch).  The folded PSP pyramid uses it (model/pspnet.py:14-31): x2 = the bilinear
 * interpolation matrix of the pooled rows (shared), w2 = the per-image pyramid terms, so that sum_s upsample(...) is two more K steps of the
 * bottleneck GEMM instead of a 92 MB tensor written by one kernel and read back as a residual by the next. */
int arseg_gemm_x3_cat_fwd(const void *x_split, const void *w_split, const void *x2_split, const void *w2_split, float *out, int M, int N, int K,
                          int K2, int out_ld, int batch, long long x_batch_stride, long long w_batch_stride, long long x2_batch_stride,
                          long long w2_batch_stride, long long out_batch_stride, const float *scale, const float *bias, int act,
                          float prelu_slope, int out_split, int tile_cfg, void *range_flag, float range_limit, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 1x1 stride-1 convolution of the 16-bit storage path as a plain GEMM of the LDS-DMA kernel (csrc/gemm_x3.hip) -- the 1x1 ConvBNReLU layers of
 * /root/reference/model/bisenet.py:162-186,335-340,387-399: out[m][co] = act(scale[co] * x[m] . w[co] + bias[co] + residual[m][co]),
 * x [M][K] / w [Cout][K] fp16 or bf16 (dtype: enum arseg_dtype; K % 64 == 0, dense rows), out / residual 16-bit with row strides out_ld / res_ld
 * (elements; a channel slice of a wider tensor is fine), scale / bias fp32 (NULL: 1 / 0), Cout % 4 == 0, 16-byte aligned pointers.
 * tile_cfg 0-11 (0-6 as arseg_gemm_x3_fwd, 7-11 narrow tiles for Cout = 64 / 128); none is chosen for the caller.
 * (Round 5's implicit-3x3 entry points on zero-bordered rows, arseg_conv3x3_rows_fwd / arseg_pad_rows_fwd, were removed in ABI v5: never selected.)
 * ------------------------------------------------------------------------------------------- */
int arseg_gemm_rows16_fwd(const void *x_rows, const void *w_rows, void *out, int dtype, long long M, int K, int Cout, int out_ld, const float *scale,
                          const float *bias, const void *residual, int res_ld, int act, float prelu_slope, int tile_cfg, arseg_stream_t stream);

/* conv3x3 (pad 1, stride 1) of a x2 bilinear (align_corners=False) upsample -- PSPUpsample, /root/reference/model/pspnet.py:43-46 --
 * by tap decomposition: since a 1x1 conv commutes with a per-channel resize, conv3x3(Up(x)) = sum_t shift_t(Up(W_t x)).  The caller
 * runs ONE 1x1 conv at low resolution with the nine taps stacked along the output channels (weights [9*Cout][Cin], row t*Cout + co =
 * W[co][.][t/3][t%3]; arseg_conv2d_fwd, no epilogue) into z = [N,h,w,9*Cout] (row stride z_ld), and this entry point samples the nine
 * planes at the shifted positions of the never-materialised upsampled image (zero outside it = the conv's padding), sums them and applies
 * out = act(scale * sum + bias) into out = [N,2h,2w,Cout].  Same multiply count as Winograd F(4x4,3x3) on the upsampled image, without
 * its transformed operand (9x the low-resolution input) and without its rounding amplification.  Cout % 4 == 0, 16-byte aligned. */
int arseg_upconv3x3_tap_gather_fwd(const float *z, int z_ld, const float *scale, const float *bias, float *out, int out_ld, int N, int h,
                                   int w, int Cout, int act, float prelu_slope, arseg_stream_t stream);
/* The same gather with its output written as split rows [N, 2h, 2w, Cout] (Cout % 32 == 0; the operand format of arseg_gemm_x3_fwd): the next
 * layer is again a tap-decomposed PSPUpsample whose low-resolution GEMM stages them by LDS-DMA (up_1 -> up_2).  range_flag / range_limit as in
 * arseg_split_rows_fwd. */
int arseg_upconv3x3_tap_gather_split_fwd(const float *z, int z_ld, const float *scale, const float *bias, void *out_split, int N, int h, int w,
                                         int Cout, int act, float prelu_slope, void *range_flag, float range_limit, arseg_stream_t stream);
int arseg_wino43_pack_weight_host(const float *w_oihw, int Cout, int Cin, float *out_host);


/* Host-side weight preparation (the "weight packer"; CPU pointers).
 * arseg_packed_k: padded GEMM depth for a conv (multiple of 32).
 * arseg_pack_conv_weight_host: OIHW [Cout][Cin][R][S] -> [Cout][Kpad], k = (r*S+s)*Cin_pad + ci, zero padded.
 * arseg_fold_bn_host: scale = gamma/sqrt(var+eps), bias = beta + (conv_bias - mean)*scale  (conv_bias may be NULL).
 * arseg_pack_dw3x3_host: depthwise [C][1][3][3] -> [9][C]. */
int arseg_packed_k(int Cin_pad, int R, int S);
int arseg_pack_conv_weight_host(const float *w_oihw, int Cout, int Cin, int R, int S, int Cin_pad, float *out_host);
/* arseg_split_weight_f16x3_host: [Cout][Kpad] fp32 (from arseg_pack_conv_weight_host / arseg_wino43_pack_weight_host rows)
 * -> ARSEG_MATH_F16X3 operand format (same byte count: per 32-k tile 32 hi halves then 32 lo halves), each row multiplied
 * by a power of two; chan_mul_inv[Cout] receives the inverse factors (multiply them into the epilogue scale); NULL = no scaling. */
int arseg_split_weight_f16x3_host(const float *w_packed_host, int Cout, int Kpad, void *out_host, float *chan_mul_inv);
int arseg_fold_bn_host(const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                       const float *conv_bias, int C, float *scale_out, float *bias_out);
int arseg_pack_dw3x3_host(const float *w, int C, float *out_host);

/* ---------------------------------------------------------------------------------------------
 * Small NHWC layers of the backbones.
 * ------------------------------------------------------------------------------------------- */
/* nn.MaxPool2d(3, stride 2, padding 1)             model/extractors.py:116, model/bisenet.py:77 */
int arseg_maxpool3x3s2_fwd(const float *in, float *out, int N, int H, int W, int C, arseg_stream_t stream);
/* nn.AdaptiveAvgPool2d((oh,ow))                                            model/pspnet.py:23
 * out[n][bin][c] at out + n*out_n_stride + bin*out_ld + c (0 = dense defaults: out_ld = C, out_n_stride = oh*ow*C),
 * so several pyramid levels can be pooled straight into one block-structured matrix. */
int arseg_adaptive_avgpool_fwd(const float *in, int in_ld, float *out, int out_ld, long long out_n_stride, int N, int H, int W,
                               int C, int oh, int ow, arseg_stream_t stream);
/* The same into one column block of a block-structured matrix [N][rows][n_blocks*C] (the folded PSP pyramid, model/pspnet.py:14-31):
 * level `block` writes its pooled map into columns [block*C, (block+1)*C) of its oh*ow rows and ZEROS into the other blocks of those
 * rows -- no fill launch.  `out` = the level's first row in image 0 (column 0 of the matrix), out_n_stride = elements between images. */
int arseg_adaptive_avgpool_blockrow_fwd(const float *in, int in_ld, float *out, long long out_n_stride, int N, int H, int W, int C,
                                        int oh, int ow, int n_blocks, int block, arseg_stream_t stream);
/* The whole pooled matrix of the folded pyramid in one pass over the map: out [N][rows][n_sizes * C], rows = sum sizes[i]^2, identical to n_sizes
 * calls of arseg_adaptive_avgpool_blockrow_fwd up to the order of summation (every bin is a union of cells of the grid spanned by all bin
 * edges; the cells are summed once, 1 / 4 of the reads).  sizes[i] <= 6, n_sizes <= 4; workspace = arseg_psp_pool_matrix_workspace_bytes. */
size_t arseg_psp_pool_matrix_workspace_bytes(int N, int H, int W, int C, int n_sizes, const int *sizes);
int arseg_psp_pool_matrix_fwd(const float *in, int in_ld, float *out, void *workspace, size_t workspace_bytes, int N, int H, int W, int C,
                              int n_sizes, const int *sizes, arseg_stream_t stream);
/* PSPModule priors (model/pspnet.py:27-30), folded: with t[n][off_s + i][c] the per-level maps AFTER the stage conv and
 * the level's slice of the bottleneck conv (both 1x1, i.e. linear and commuting with bilinear upsampling), this writes
 * out[n,y,x,c] = sum_s upsample_bilinear(align_corners=False)(t_s[n])(y,x,c); off_s = sum_{j<s} sizes[j]^2 (host array). */
int arseg_psp_prior_sum_fwd(const float *t, float *out, int N, int H, int W, int C, int n_sizes, const int *sizes_host,
                            arseg_stream_t stream);
/* torch.mean(x,(2,3)) / F.adaptive_max_pool2d(x,1): out [N][C]   model/bisenet.py:252,292,390; pspnet.py:94 */
int arseg_global_reduce_fwd(const float *in, int in_ld, float *out, int N, int H, int W, int C, int op,
                            arseg_stream_t stream);
/* The same reduction with a caller-owned workspace (arseg_global_reduce_workspace_bytes, 0 = not needed): a large map of few images (the keyframe's
 * auxiliary head) is reduced in two deterministic stages -- row bands into the workspace, then the bands in order -- so that the whole chip reads it. */
size_t arseg_global_reduce_workspace_bytes(int N, int H, int W, int C);
int arseg_global_reduce_ws_fwd(const float *in, int in_ld, float *out, void *workspace, size_t workspace_bytes, int N, int H, int W, int C, int op,
                               arseg_stream_t stream);
/* F.interpolate / F.upsample / nn.Upsample: nearest or bilinear, align_corners on/off, either layout.
 * NHWC: in_ld/out_ld channel strides (C % 4 == 0); NCHW: planes contiguous, ld arguments ignored.
 * model/pspnet.py:29,45,97; model/bisenet.py:215,284,298,442; evaluation.py:117,188,201 */
int arseg_resize_fwd(const float *in, float *out, int N, int C, int Hin, int Win, int Hout, int Wout, int mode,
                     int align_corners, int layout, int in_ld, int out_ld, arseg_stream_t stream);
/* out[n,y,x,c] = x[n,y,x,c] * scale[n,c] + (add_full ? add_full[n,y,x,c] : 0) + (add_vec ? add_vec[n,c] : 0)
 * ARM: feat*atten (+avg)  model/bisenet.py:258,295;  FFM: feat*atten + feat  model/bisenet.py:397-398 */
int arseg_scale_add_fwd(const float *x, const float *scale, const float *add_full, const float *add_vec, float *out,
                        int N, int HW, int C, arseg_stream_t stream);
/* final 1x1 classifier on an NHWC feature, NCHW logits out (+ optional LogSoftmax over classes)
 * model/pspnet.py:66-67,96-98; model/bisenet.py:211,448 */
int arseg_head_fwd(const float *p, int p_ld, const float *wf, const float *bf, float *logits, int N, int HW, int C,
                   int n_cls, int log_softmax, arseg_stream_t stream);
/* decoded frame NCHW [N,3,H,W] -> NHWC4 [N,h,w,4] (4th channel 0), bilinear align_corners=True when (h,w) != (H,W)
 * evaluation.py:115-117,186-188 fused with the layout change the conv engine wants */
int arseg_frame_to_nhwc4_fwd(const float *img, float *out, int N, int H, int W, int h, int w, arseg_stream_t stream);
/* Decoded uint8 HWC frame(s) [N,H,W,3] (device) -> normalised NHWC4 at (h,w): ToTensor + Normalize(mean, std)
 * (dataset/camvid.py:503-506, dataset/cityscapes.py:208-214) + the evaluator's bilinear align_corners=True downscale
 * (evaluation.py:186-188) in one pass.  mean3 / std3: host pointers to 3 floats. */
int arseg_frame_u8_to_nhwc4_fwd(const uint8_t *img_hwc, float *out, int N, int H, int W, int h, int w, const float *mean3,
                                const float *std3, arseg_stream_t stream);
/* 8-bit decoder frames -> the conv engine's input in one pass, no intermediate tensor (csrc/ingest.hip).
 *   src_format  ARSEG_SRC_RGB8: plane0 = uint8 [N][H][W][3] interleaved (the layout arseg_frame_u8_to_nhwc4_fwd takes); plane1, pitch1,
 *                               n_stride1 and colour are ignored
 *               ARSEG_SRC_NV12: plane0 = luma uint8 [N][H][W], plane1 = chroma uint8 [N][H/2][W/2][2] (Cb, Cr interleaved); H and W even
 *   pitch0/1    bytes from one row of the plane to the next (>= 3 W for RGB8, >= W for either NV12 plane); n_stride0/1: bytes from one
 *               image to the next (>= 0; 0 = every image reads the same plane).  Rows may be padded; nothing past a row's last pixel is read.
 *   out         out_dtype ARSEG_DT_F32: NHWC4 fp32 [N][h][w][4], channel 3 = 0;  ARSEG_DT_F16 | ARSEG_DT_BF16: NHWC8 [N][h][w][8],
 *               channels 3..7 = 0.  16-byte aligned.
 *   mean3/std3  host pointers to 3 floats (dataset/camvid.py:503-506).
 * Per output pixel, all in fp32: (1) the taps of F.interpolate(..., (h, w), mode='bilinear', align_corners=True) on the H x W frame
 * (evaluation.py:117,188), as the other ingest kernels compute them; (h, w) == (H, W) reads one tap and blends nothing; h > H or w > W
 * upscales with the same formula.  (2) RGB in the 0-255 scale at each tap -- RGB8: the stored bytes.  NV12: Y = the stored byte; (Cb, Cr)
 * sampled bilinearly from the half-resolution plane at the luma pixel's position under the H.26x default chroma siting (co-sited with
 * even luma columns, midway between two luma rows): cx = x / 2, cy = y / 2 - 0.25, both clamped to the plane; then
 *       R = ky (Y - y0) + rv (Cr - 128),   G = ky (Y - y0) - gu (Cb - 128) - gv (Cr - 128),   B = ky (Y - y0) + bu (Cb - 128)
 *       rv = 2 (1 - Kr) s,  bu = 2 (1 - Kb) s,  gu = 2 Kb (1 - Kb) / Kg s,  gv = 2 Kr (1 - Kr) / Kg s,  Kg = 1 - Kr - Kb
 *       BT.601: Kr = 0.299, Kb = 0.114;  BT.709: Kr = 0.2126, Kb = 0.0722
 *       limited range (Y 16-235, C 16-240): y0 = 16, ky = 255 / 219, s = 255 / 224;   full range: y0 = 0, ky = 1, s = 1
 *         colour                        ky        rv        gu        gv        bu
 *         ARSEG_COLOUR_BT601_LIMITED    1.164384  1.596027  0.391762  0.812968  2.017232
 *         ARSEG_COLOUR_BT601_FULL       1         1.402     0.344136  0.714136  1.772
 *         ARSEG_COLOUR_BT709_LIMITED    1.164384  1.792741  0.213249  0.532909  2.112402
 *         ARSEG_COLOUR_BT709_FULL       1         1.5748    0.187324  0.468124  1.8556
 *     each component clipped to [0, 255], not rounded to an integer.  (3) the taps are blended, then (v / 255 - mean[c]) / std[c]
 * (evaluated as one fma with 1 / (255 std) and -mean / std formed in double; within 2 ulp of the two divisions).  16-bit outputs are
 * rounded once, at the store (to nearest even).  One kernel family serves this entry point and arseg_frame_ingest_yuv_fwd; apart from that
 * fma and the tap weight's, no multiply is fused with an add, so the fp32 result does not depend on the format, the route or the output type.
 * ARSEG_EINVAL: a null pointer (plane1 only with NV12), a non-positive size, a zero std, odd H or W with NV12, a pitch smaller than a
 * row, a negative image stride, an unknown src_format / out_dtype / colour (colour with NV12 only), `out` not 16-byte aligned. */
enum arseg_src_format { ARSEG_SRC_RGB8 = 0, ARSEG_SRC_NV12 = 1, ARSEG_SRC_I420 = 2, ARSEG_SRC_P010 = 3, ARSEG_SRC_I010 = 4 };     /* 2..4: arseg_frame_ingest_yuv_fwd */
enum arseg_colour { ARSEG_COLOUR_BT601_LIMITED = 0, ARSEG_COLOUR_BT601_FULL = 1, ARSEG_COLOUR_BT709_LIMITED = 2, ARSEG_COLOUR_BT709_FULL = 3 };
int arseg_frame_ingest_fwd(const void *plane0, const void *plane1, int src_format, int64_t pitch0, int64_t pitch1, int64_t n_stride0,
                           int64_t n_stride1, int colour, void *out, int out_dtype, int N, int H, int W, int h, int w, const float *mean3,
                           const float *std3, arseg_stream_t stream);
/* Planar 4:2:0 and 10-bit decoder frames -> the conv engine's input, the same pass as arseg_frame_ingest_fwd (csrc/ingest.hip).
 *   src_format  ARSEG_SRC_I420: plane0 = Y uint8 [N][H][W], plane1 = Cb uint8 [N][H/2][W/2], plane2 = Cr uint8 [N][H/2][W/2]
 *                               (what a software HEVC decoder hands over for a yuv420p stream)
 *               ARSEG_SRC_P010: plane0 = Y uint16 [N][H][W], plane1 = (Cb, Cr) interleaved uint16 [N][H/2][W/2][2], plane2 / pitch2 /
 *                               n_stride2 ignored; little-endian words, code = word >> 6 (the low 6 bits are ignored)
 *               ARSEG_SRC_I010: planes as I420 with uint16 little-endian samples (yuv420p10le), code = word & 0x3ff (the high 6 bits
 *                               are ignored)
 *               ARSEG_SRC_RGB8 and ARSEG_SRC_NV12 are unknown to this entry point: they keep arseg_frame_ingest_fwd.
 *   pitch0/1/2, n_stride0/1/2   bytes, per plane, as above; a row holds W (I420 Y), 2 W (16-bit Y, P010 chroma), W / 2 (I420 chroma) or
 *               W (I010 chroma) bytes.  Rows may be padded; nothing past a row's last sample is read.  H and W even.  Pointer, pitch and
 *               image stride of a 16-bit plane are even.
 *   colour, out, out_dtype, mean3 / std3: as arseg_frame_ingest_fwd.
 * Contract: steps (1) and (3) of arseg_frame_ingest_fwd unchanged, and so is the chroma siting (cx = x / 2, cy = y / 2 - 0.25, clamped to
 * the plane, bilinear on the stored codes).  Step (2) gains the bit depth n = 8 (I420) or 10 (P010, I010): with C = the interpolated
 * chroma code,
 *       limited range:  Y8 = code_Y 2^-(n-8),          C8 - 128 = (C - 2^(n-1)) 2^-(n-8)          (10-bit: Y 64-940, C 64-960; exact in fp32)
 *       full range (H.273):  Y8 = code_Y 255 / (2^n - 1),   C8 - 128 = (C - 2^(n-1)) 255 / (2^n - 1)   (the factor formed in double, rounded
 *                                                                                                     to fp32 once; 1 for n = 8)
 * then the matrix of `colour` on (Y8 - y0, C8b - 128, C8r - 128) as above, each component clipped to [0, 255], not rounded.  For equal
 * sample values the three formats, and NV12 through arseg_frame_ingest_fwd, give the same fp32 bits.  BT.2020, 12-bit, 4:2:2 and 4:4:4 sources are not covered.
 * ARSEG_EINVAL: a null pointer (plane2 with the planar formats only), a non-positive size, odd H or W, a pitch smaller than a row, a
 * negative image stride, an odd pointer / pitch / image stride of a 16-bit plane, a zero std, an unknown src_format / out_dtype / colour,
 * `out` not 16-byte aligned. */
int arseg_frame_ingest_yuv_fwd(const void *plane0, const void *plane1, const void *plane2, int src_format, int64_t pitch0, int64_t pitch1,
                               int64_t pitch2, int64_t n_stride0, int64_t n_stride1, int64_t n_stride2, int colour, void *out, int out_dtype,
                               int N, int H, int W, int h, int w, const float *mean3, const float *std3, arseg_stream_t stream);

/* mergeMotion (pre-process/generate_compressed_dataset_camvid.py:6-56): chains the codec's per-frame motion fields back to
 * the keyframe.  flows: int16 [n_frames+1][H][W][3] = (mv_x, mv_y quarter-pel, reference index), entries <= frame_start unused;
 * out: int16 [n_frames+1][H][W][2], frame f > 0 = accumulated quarter-pel motion of frame f to the keyframe (what the
 * datasets' .bin files hold), frame 0 = -1 as in the reference.  workspace: arseg_merge_motion_workspace_bytes() bytes. */
size_t arseg_merge_motion_workspace_bytes(int n_frames, int H, int W);
int arseg_merge_motion_fwd(const int16_t *flows, int16_t *out, void *workspace, size_t workspace_bytes, int n_frames, int frame_start,
                           int H, int W, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder motion-vector block records -> mv_q, chained to the keyframe frame by frame (csrc/mv_records.hip).
 * The motion half of a decoder's output as a decoder holds it (libde265's prediction-unit table, FFmpeg's motion-vector side data): a
 * list of block records per P-frame instead of mergeMotion's dense per-frame dumps, consumed one frame at a time.
 *   record      16 bytes, 16-byte aligned, eight int16:  x, y, w, h, mvx, mvy, ref, reserved
 *                 x, y      top-left luma pixel of the block
 *                 w, h      its size in pixels
 *                 mvx, mvy  quarter-pel displacement from the block to its reference position, mergeMotion's sign: k2 = k1 + round(mvx / 4)
 *                 ref       reference index as mergeMotion reads channel 2: 0 = the previous frame, r = r + 1 frames back;
 *                           ref < 0 or ref >= max_ref = intra
 *                 reserved  ignored, whatever it holds
 *   records     int16 [n_records][8] on the device; n_records is a host integer, the CAPACITY of the buffer (may be 0, then records may
 *               be NULL)
 * Rasterisation (one frame's records -> one dense field):
 *   - a record covers the integer rectangle [x, x + w) x [y, y + h) clipped to the frame; any position and size, on or off the frame
 *   - w <= 0 or h <= 0 covers nothing: a fixed-capacity buffer padded with zero records is valid, and a HIP graph captured over such a
 *     buffer can be replayed on refilled contents
 *   - where records overlap the HIGHEST record index wins (deterministic: an atomic maximum of the index, not the arrival order)
 *   - a pixel no record covers reads (0, 0, -1): intra
 * Chaining = mergeMotion with frame_start = 0 (pre-process/generate_compressed_dataset_camvid.py:6-56), per pixel (x, y) of frame f >= 1:
 *       intra -> (mvx, mvy, ref) = (0, 0, 0)                                    (:20-22, with max_ref in place of the constant 3)
 *       k2 = clamp(x + round(mvx / 4), 0, W - 1),  j2 = clamp(y + round(mvy / 4), 0, H - 1)      round = np.round: half to even (:26-34)
 *       f2 = max(0, f - ref - 1)                                                                                               (:28)
 *       merged[f][y][x] = 4 (k2 - x, j2 - y) + (f2 > 0 ? merged[f2][j2][k2] : (0, 0))       (a pixel links to its target's link, :37-54)
 *   H, W <= 8192: every accumulated value is then at most 4 * 8191 in magnitude and fits int16 without wrapping, which is what lets the
 *   merged tensor itself be the chain state (mergeMotion's per-pixel link table, 16 bytes per pixel and frame, is not needed).
 *   merged: int16 [gop][H][W][2], caller-owned, 4-byte aligned; frames 1 .. f of it are the mv_q the warp entry points above take.
 * Entry points (enqueue only: no host synchronisation, no allocation):
 *   arseg_mv_records_workspace_bytes  one int32 index map: 4 H W bytes (0 for a size outside 1 .. 8192)
 *   arseg_mv_records_reset            starts a GOP: index map = -1, merged[0] = -1 (what arseg_merge_motion_fwd leaves in frame 0, so the
 *                                     whole tensor compares bit for bit)
 *   arseg_mv_records_step_fwd         one P-frame f in [1, gop): reads merged[f2] for f2 < f, writes merged[f]; leaves the index map at -1.
 *                                     Frames must be pushed in order 1, 2, ... after a reset.  max_ref in 1 .. 16 (the reference's constant: 3)
 *   arseg_mv_records_rasterize_fwd    the dense field alone, dense_out int16 [H][W][3] = (mvx, mvy, ref) of the winning record as stored
 *                                     (no intra rule), for cross-checks and for writing the reference's dumps; the workspace needs no
 *                                     reset before it and is left at -1
 * workspace: 16-byte aligned, >= arseg_mv_records_workspace_bytes(H, W) bytes (else ARSEG_EWORKSPACE).
 * ARSEG_EINVAL: a null pointer, n_records < 0, H or W outside 1 .. 8192, max_ref outside 1 .. 16, f outside [1, gop), records or workspace
 * not 16-byte aligned, merged not 4-byte aligned.  B-frames (two records per block, forward references, decode order) are outside these
 * entry points: arseg_mv_records_bi_* below take them.
 * ------------------------------------------------------------------------------------------- */
size_t arseg_mv_records_workspace_bytes(int H, int W);
int arseg_mv_records_reset(int16_t *merged, void *workspace, size_t workspace_bytes, int H, int W, arseg_stream_t stream);
int arseg_mv_records_step_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, void *workspace, size_t workspace_bytes,
                              int H, int W, int max_ref, arseg_stream_t stream);
int arseg_mv_records_rasterize_fwd(const int16_t *records, int n_records, int16_t *dense_out, void *workspace, size_t workspace_bytes, int H,
                                   int W, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * B-frame motion records: two prediction lists per frame, references before and after the frame, frames pushed in DECODE order
 * (csrc/mv_records.hip).  mergeMotion has no rule for this case; the rule below is this library's, written so that a P-only stream pushed
 * in display order gives arseg_mv_records_step_fwd's result bit for bit under every policy.
 *   record      the same 16 bytes; two fields read differently:
 *                 ref       signed display-order offset code from frame f: 0 <= ref < max_ref -> target t = max(0, f - ref - 1) as above;
 *                           -max_ref <= ref < 0 -> t = f - ref (-1 = the next frame in display order); any other value: the record is UNUSABLE
 *                 reserved  bit 0 = the prediction list (0 or 1), every other bit ignored.  A list is not a direction: list 0 may point
 *                           forward, list 1 backward, both the same way (low-delay B)
 * Per frame f, pushed with the set D of frames already chained in this GOP (done_mask: bit g set = g in D; 0 in D always, f not in D):
 *   - per list l the winner at a pixel is the HIGHEST record index among the records of that list covering it; clipping, w <= 0 or h <= 0
 *     padding and off-frame positions exactly as in the rasterisation rules above
 *   - a winner is USABLE if its ref is in range and its target t_l is in D.  An unusable winner does not fall back to a lower index (as an
 *     intra record covers pixels above)
 *   - link_l = 4 (k2 - x, j2 - y) + (t_l > 0 ? merged[t_l][j2][k2] : (0, 0)),  k2 = clamp(x + round(mvx / 4), 0, W - 1), j2 likewise, round = half to even
 *   - exactly one list usable: merged[f][y][x] = that list's link
 *   - neither usable (intra): p = max{g in D : g < f}, merged[f][y][x] = p > 0 ? merged[p][y][x] : (0, 0) -- zero motion to the nearest chained
 *     frame before f; with in-order pushes the intra rule above
 *   - both usable, by `policy`:
 *       ARSEG_MVR_BI_LIST0  link_0
 *       ARSEG_MVR_BI_NEAR   the list with the smaller |t_l - f|, a tie goes to list 0
 *       ARSEG_MVR_BI_MEAN   per component (link_0 + link_1) / 2 rounded half to even (int16 and inside the frame because both ends are)
 * Entry points (enqueue only: no host synchronisation, no allocation):
 *   arseg_mv_records_bi_workspace_bytes  two int32 index maps, one per list: 8 H W bytes (0 for a size outside 1 .. 8192)
 *   arseg_mv_records_bi_reset            starts a GOP: both maps = -1, merged[0] = -1
 *   arseg_mv_records_bi_step_fwd         one frame f in [1, gop): reads merged[t] for t in D, writes merged[f], leaves both maps at -1.  Two
 *                                        launches.  done_mask is a kernel argument: a captured HIP graph replays one fixed decode order, which
 *                                        is what a GOP structure is.  merged, records, workspace alignment and n_records as above
 * ARSEG_EINVAL before any launch: everything arseg_mv_records_step_fwd refuses; gop > 64; bit 0 of done_mask clear; bit f of done_mask set; a
 * bit >= gop of done_mask set; policy outside 0 .. 2.  ARSEG_EWORKSPACE: workspace_bytes below arseg_mv_records_bi_workspace_bytes(H, W).
 * Not covered: open GOPs (references across a keyframe), choosing the path with the fewest hops to the keyframe, weighted prediction, more
 * than one keyframe per chain.
 * ------------------------------------------------------------------------------------------- */
enum arseg_mvr_bi_policy { ARSEG_MVR_BI_LIST0 = 0, ARSEG_MVR_BI_NEAR = 1, ARSEG_MVR_BI_MEAN = 2 };
size_t arseg_mv_records_bi_workspace_bytes(int H, int W);
int arseg_mv_records_bi_reset(int16_t *merged, void *workspace, size_t workspace_bytes, int H, int W, arseg_stream_t stream);
int arseg_mv_records_bi_step_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, uint64_t done_mask, int policy,
                                 void *workspace, size_t workspace_bytes, int H, int W, int max_ref, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Link quality along the chain (csrc/mv_records.hip): merged keeps the accumulated displacement of a pixel and nothing about how good its
 * links are.  Three things that happen at a hop all end as an ordinary-looking vector: an INTRA block (the encoder found no usable
 * prediction; the rule substitutes zero motion), an UNCOVERED pixel (no record; the same substitution) and a CLAMPED target (it fell off
 * the frame and was pulled back to the border).  The link entry points write, next to merged[f], one byte per pixel that keeps them.
 *   link        uint8 [gop][H][W] on the device, contiguous, caller-owned; frame 0 is all zero.  For frame f and pixel (x, y), flag bits
 *               mean "at this hop or at any hop between here and the keyframe":
 *                 bit 0  ARSEG_LINK_INTRA      set at a hop when a record won the pixel but could not be used.  P entry: ref < 0 or ref >= max_ref.
 *                                              Bi entry: no list is usable and at least one list has a winner (its ref out of range or its
 *                                              target not in D)
 *                 bit 1  ARSEG_LINK_UNCOVERED  no record of any list covers the pixel (index outside [0, n_records))
 *                 bit 2  ARSEG_LINK_CLAMPED    a USED list's rounded target x + round_half_even_div4(mvx) or y + round_half_even_div4(mvy) lay
 *                                              outside the frame before the clamp
 *                 bit 3  reserved, written 0
 *                 bits 4..7  hops: the number of links from this pixel to the keyframe, saturating at 15; a pixel whose target is in frame
 *                            0 has 1 hop
 *   Propagation, with (t, j2, k2) EXACTLY the pixel whose merged value the compose step gathers (the intra / uncovered substitution targets
 *   the same pixel of frame max(0, f - 1), P entry, or of frame p, bi entry, as in the rules above), and g = t > 0 ? link[t][j2][k2] : 0:
 *       link[f][y][x] = ((own flags | g) & 7) | (min(15, 1 + (g >> 4)) << 4)
 *   Bi entry under LIST0 / NEAR: only the chosen list contributes.  Under MEAN with both lists usable: the flags are the OR of both lists'
 *   bytes, the hops their maximum.  With every record in list 0, frames pushed in order and done_mask = (1 << f) - 1 the bi entry's link
 *   equals the P entry's bit for bit under every policy, as merged does.
 *   link_stats  int64 [gop][ARSEG_LINK_NSTATS] on the device, 8-byte aligned, may be NULL; row f is ACCUMULATED INTO by the step of frame f:
 *                 [0] pixels with INTRA   [1] with UNCOVERED   [2] with CLAMPED   [3] with any flag   [4 + h] pixels with h hops (h = 0 .. 15)
 *               Integers: two runs are bit-equal.
 * Entry points (enqueue only: no host synchronisation, no allocation; a captured graph replays them):
 *   arseg_mv_link_reset                zeroes link[0] and every row of link_stats (if not NULL); one launch.  Goes with arseg_mv_records_reset
 *                                      / _bi_reset, which it does not replace
 *   arseg_mv_records_step_link_fwd     arseg_mv_records_step_fwd + link, link_stats: writes merged[f] bit-equal to that entry, and link[f].
 *                                      No further launch: the compose pass writes the byte (a 1-byte gather at the address pattern of the
 *                                      4-byte one)
 *   arseg_mv_records_bi_step_link_fwd  the same for arseg_mv_records_bi_step_fwd
 * ARSEG_EINVAL before any launch: everything the plain entries refuse; a null link; a link_stats that is not 8-byte aligned; reset: gop < 1,
 * H or W outside 1 .. 8192.
 * Not covered: which hop set a flag; a per-list byte under MEAN; link bytes for arseg_merge_motion_fwd's dense route.
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_LINK_INTRA 1
#define ARSEG_LINK_UNCOVERED 2
#define ARSEG_LINK_CLAMPED 4
#define ARSEG_LINK_NSTATS (4 + 16)
int arseg_mv_link_reset(uint8_t *link, int64_t *link_stats, int gop, int H, int W, arseg_stream_t stream);
int arseg_mv_records_step_link_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, void *workspace, size_t workspace_bytes,
                                   int H, int W, int max_ref, uint8_t *link, int64_t *link_stats, arseg_stream_t stream);
int arseg_mv_records_bi_step_link_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, uint64_t done_mask, int policy,
                                      void *workspace, size_t workspace_bytes, int H, int W, int max_ref, uint8_t *link, int64_t *link_stats,
                                      arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Block motion estimation (csrc/block_motion.hip): the records above for a stream whose decoder hands over frames and no motion vectors
 * (a hardware decoder's NV12 / P010 output).  Full search of every block of the current frame's luma in a reference frame's, 8-bit integer
 * arithmetic throughout; the records go to arseg_mv_records_step_fwd / _step_link_fwd as a software decoder's would.
 *   luma8       of a sample, by src_format (enum arseg_src_format), taken while the planes are read -- there is no conversion pass:
 *                 ARSEG_SRC_NV12, ARSEG_SRC_I420   the luma byte
 *                 ARSEG_SRC_I010                   (v & 0x3ff) >> 2       (uint16 little endian, code in the low 10 bits)
 *                 ARSEG_SRC_P010                   v >> 8                 (code in the high 10 bits)
 *                 ARSEG_SRC_RGB8                   (77 R + 150 G + 29 B + 128) >> 8
 *               Chroma is not read.
 *   cur, ref    the luma plane ([H][W] samples) of the current and of the reference frame -- for ARSEG_SRC_RGB8 the interleaved plane
 *               ([H][W][3] bytes) -- on the device, rows cur_pitch / ref_pitch BYTES apart; read only
 *   blocks      H, W in 1 .. 8192, B in {8, 16}: by = ceil(H / B) rows of bx = ceil(W / B) blocks.  Block (bi, bj): x0 = bj B, y0 = bi B,
 *               w = min(B, W - x0), h = min(B, H - y0); it is record bi * bx + bj.  Always exactly by * bx records.
 *   candidates  every integer (dx, dy), |dx| <= R and |dy| <= R, R in 1 .. 32, whose displaced block lies inside the reference frame:
 *               0 <= x0 + dx, x0 + w + dx <= W, 0 <= y0 + dy, y0 + h + dy <= H.  (0, 0) always is one.  No sample is padded or clamped, so
 *               the chain never sets ARSEG_LINK_CLAMPED for an estimated record.
 *   cost        SAD(dx, dy) = sum over the block's w h pixels of |luma8(cur[y][x]) - luma8(ref[y + dy][x + dx])|
 *               cost = SAD + lambda (|dx| + |dy|), lambda in 0 .. 255
 *   winner      the candidate with the smallest (cost, rank), rank(0, 0) = 0, otherwise rank = 1 + (dy + R)(2 R + 1) + (dx + R)
 *               (cost < 2^17 and rank < 2^13: one unsigned minimum of cost << 13 | rank decides)
 *   record      (x0, y0, w, h, 4 dx, 4 dy, ref_index, 0), ref_index in 0 .. 15 (0 = `ref` is the previous frame); if the winner's
 *               SAD > intra w h (intra in 0 .. 255: a mean absolute difference per pixel; SAD == intra w h is a match, 255 never fires):
 *               (x0, y0, w, h, 0, 0, ARSEG_BM_INTRA_REF, 0) -- 16 is unusable for every max_ref <= 16, so both chain entries flag the
 *               block's pixels ARSEG_LINK_INTRA
 *   records     int16 [by * bx][8] on the device, 16-byte aligned; every record is written
 *   sad         uint32 [by * bx], may be NULL: the winner's SAD (of intra blocks too)
 *   stats       int64 [ARSEG_BM_NSTATS], 8-byte aligned, may be NULL; ACCUMULATED INTO: [0] intra blocks, [1] matched blocks with the zero
 *               vector, [2] sum of SAD over matched blocks, [3] pixels in matched blocks.  Integers: two runs are bit-equal.
 * Entry points (enqueue only: no host synchronisation, no allocation; one launch, a captured graph replays it):
 *   arseg_block_motion_workspace_bytes  0: the search lives in LDS and registers.  Kept so that a caller sizes the workspace as elsewhere
 *   arseg_block_motion_fwd              workspace may be NULL while the function above answers 0
 * ARSEG_EINVAL before any launch: a null cur, ref or records; H or W outside 1 .. 8192; B outside {8, 16}; R outside 1 .. 32; lambda or
 * intra outside 0 .. 255; ref_index outside 0 .. 15; an unknown src_format; a pitch below the row's bytes (W, 2 W for the 16-bit formats,
 * 3 W for RGB8); a pitch or plane pointer that is odd with a 16-bit format; records not 16-byte, sad not 4-byte, stats not 8-byte aligned.
 * ARSEG_EWORKSPACE: workspace_bytes below arseg_block_motion_workspace_bytes(H, W, B, R).
 * Not covered: sub-pel refinement (the chain rounds every hop to whole pixels), variable block sizes (16 x 16 blocks split into 8 x 8 where
 * that pays: arseg_block_motion_split_fwd below), two references per block, chroma.  (Reach beyond 32 pixels: the hierarchical search below.)
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_BM_INTRA_REF 16
#define ARSEG_BM_NSTATS 4
size_t arseg_block_motion_workspace_bytes(int H, int W, int B, int R);
int arseg_block_motion_fwd(const void *cur, int64_t cur_pitch, const void *ref, int64_t ref_pitch, int src_format, int H, int W, int B, int R,
                           int lambda, int intra, int ref_index, int16_t *records, uint32_t *sad, int64_t *stats, void *workspace,
                           size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Hierarchical block motion search (csrc/block_motion_pyr.hip): the same records from a coarse-to-fine search over a luma8 pyramid --
 * a reach of Rt 2^L + r (2^L - 1) pixels for about a hundredth of the full search's SADs.  All integers: two runs are bit-equal.
 *   pyramid     P_0 = the luma8 plane of the source (formats and luma8 as above), H_0 x W_0 = H x W in 1 .. 8192; for l = 0 .. L - 1,
 *               L = levels in 1 .. 3:  H_{l+1} = (H_l + 1) >> 1, W_{l+1} = (W_l + 1) >> 1,
 *               P_{l+1}[y][x] = (a + b + c + d + 2) >> 2 over P_l[min(2 y + i, H_l - 1)][min(2 x + j, W_l - 1)], i, j in {0, 1}
 *               (the last row / column is replicated where a size is odd)
 *   buffer      uint8 on the device, 16-byte aligned: level l at byte offset off_l, rows pitch_l = (W_l + 15) & ~15 bytes apart, off_0 = 0,
 *               off_{l+1} = off_l + pitch_l H_l; arseg_luma_pyramid_bytes = off_{L+1}.  Level 0 is materialised, so the search reads bytes
 *               whatever the source format was.  The bytes of a row beyond W_l are unspecified and never count as pixels; nothing
 *               beyond the total is touched.
 *   block grids level l has by_l = ceil(H_l / B) rows of bx_l = ceil(W_l / B) blocks of B x B level-l pixels, B in {8, 16}, clipped at the
 *               right and bottom edge as above; the grid of level 0 is the record grid above.  Block (bi, bj) of level l has the parent
 *               (bi >> 1, bj >> 1) at level l + 1, which always exists.
 *   top level   exactly arseg_block_motion_fwd's candidates, cost and winner on P_L(cur) against P_L(ref), of size H_L x W_L, with
 *               R = Rt in 1 .. 32 and lambda; no intra test.  This is v_L per block.
 *   refinement  for l = L - 1 .. 0, per block (bi, bj) of level l:
 *     centres     (0, 0); 2 v_{l+1} of the parent; 2 v_{l+1} of the parent's horizontal neighbour on the child's side -- parent column
 *                 (bj >> 1) + ((bj & 1) ? 1 : -1), if that column is in the grid; 2 v_{l+1} of its vertical neighbour likewise, with bi
 *     candidates  the union (a vector proposed twice counts once) of centre + (ox, oy), |ox| <= r and |oy| <= r, r in 1 .. 3, whose
 *                 displaced block lies inside P_l(ref): 0 <= x0 + dx, x0 + w + dx <= W_l, 0 <= y0 + dy, y0 + h + dy <= H_l.  Nothing is
 *                 padded or clamped.  (0, 0) always is one.
 *     cost        SAD + lambda (|dx| + |dy|), in level-l pixels
 *     winner      the smallest (cost, rank): rank(0, 0) = 0, otherwise rank = 1 + (dy + 511) 1023 + (dx + 511) -- (0, 0) first, then the
 *                 smallest dy, then the smallest dx.  (The reach at level 0 is at most 32 * 8 + 3 * 7 = 277, so rank < 2^20 and
 *                 cost < 2^19: one 64-bit minimum of cost << 20 | rank decides.)
 *   level 0     records, sad and stats as arseg_block_motion_fwd writes them: (x0, y0, w, h, 4 dx, 4 dy, ref_index, 0); SAD > intra w h
 *               -> (x0, y0, w, h, 0, 0, ARSEG_BM_INTRA_REF, 0); sad of intra blocks too; stats ACCUMULATED INTO
 *   workspace   16-byte aligned: the records of levels 1 .. L in the record format, 16 bytes per block, level 1 first (a parent's vector
 *               is fields 4 and 5 divided by 4)
 * Entry points (enqueue only: no host synchronisation, no allocation; a captured graph replays them):
 *   arseg_luma_pyramid_bytes                the size of the buffer; 0 for H, W or levels out of range
 *   arseg_luma_pyramid_fwd                  one launch for all levels; plane, pitch (bytes) and src_format as cur / cur_pitch above
 *   arseg_block_motion_pyr_workspace_bytes  16 (by_1 bx_1 + .. + by_L bx_L); 0 for H, W, B or levels out of range
 *   arseg_block_motion_pyr_fwd              levels + 1 launches on one stream, the levels top-down; cur_pyr and ref_pyr are pyramids of H x W
 *                                           frames with `levels` levels; sad and stats may be NULL
 * ARSEG_EINVAL before any launch: a null plane, pyramid, cur_pyr, ref_pyr, records or workspace; H or W outside 1 .. 8192; levels outside
 * 1 .. 3; B outside {8, 16}; Rt outside 1 .. 32; r outside 1 .. 3; lambda or intra outside 0 .. 255; ref_index outside 0 .. 15; an unknown
 * src_format; a pitch below the row's bytes; a pitch or plane pointer that is odd with a 16-bit format; a pyramid or workspace that is not
 * 16-byte aligned; records not 16-byte, sad not 4-byte, stats not 8-byte aligned; pyramid_bytes below arseg_luma_pyramid_bytes(H, W, levels).
 * ARSEG_EWORKSPACE: workspace_bytes below arseg_block_motion_pyr_workspace_bytes(H, W, B, levels).
 * Not covered: sub-pel refinement, predictors from the previous frame's field or from spatial neighbours at the same level, variable block
 * sizes (arseg_block_motion_split_fwd below splits the level-0 records), two references per block, chroma, more than three levels, caching
 * pyramids across calls (a caller keeps the buffers it built).
 * ------------------------------------------------------------------------------------------- */
size_t arseg_luma_pyramid_bytes(int H, int W, int levels);
int arseg_luma_pyramid_fwd(const void *plane, int64_t pitch, int src_format, int H, int W, int levels, uint8_t *pyramid, size_t pyramid_bytes,
                           arseg_stream_t stream);
size_t arseg_block_motion_pyr_workspace_bytes(int H, int W, int B, int levels);
int arseg_block_motion_pyr_fwd(const uint8_t *cur_pyr, const uint8_t *ref_pyr, int H, int W, int levels, int B, int Rt, int r, int lambda, int intra,
                               int ref_index, int16_t *records, uint32_t *sad, int64_t *stats, void *workspace, size_t workspace_bytes,
                               arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Keyframe anchoring of estimated block motion (csrc/block_motion_anchor.hip).  The records above are hops to the previous frame; the chain
 * composes them into the displacement to the keyframe, so a wrong hop is inherited by every later frame of the GOP, and a block that was
 * intra once stays flagged ARSEG_LINK_INTRA although its content is visible again.  The keyframe's luma is on the card: this entry checks
 * the composed displacement of every block of frame f against the keyframe directly and, where a match is found, rewrites the block's
 * record with ref = f - 1 -- target frame 0, one hop, this hop's flags only.  arseg_mv_records_step_* take the result as they are.
 *   cur, key    luma8 byte planes [H][W] of frame f and of the keyframe, rows cur_pitch / key_pitch BYTES apart; the base 4-byte aligned,
 *               the pitch a multiple of 4 and at least (W + 3) & ~3.  Level 0 of a luma pyramid qualifies, and so does an aligned NV12 /
 *               I420 luma plane.  The bytes of a row beyond W are unspecified and never count.  H, W in 1 .. 8192
 *   blocks      B in {8, 16}: the grid of arseg_block_motion_fwd; block (bi, bj) is record b = bi bx + bj of records_in and records_out,
 *               x0 = bj B, y0 = bi B, w = min(B, W - x0), h = min(B, H - y0).  Of records_in[b] only fields 4, 5 and 6 are read
 *   hop(q)      of a block q: USABLE iff field 6 of records_in[q] is 0 (the previous frame); then (hx, hy) = round_half_even_div4 of
 *               fields 4 and 5, as the chain rounds.  Otherwise (ARSEG_BM_INTRA_REF, any other index) unusable and (hx, hy) = (0, 0)
 *   pred(q)     with (xc, yc) = (x0 + w / 2, y0 + h / 2) of q, integer division: p = (clamp(xc + hx, 0, W - 1), clamp(yc + hy, 0, H - 1)),
 *               pred(q) = (hx, hy) + (merged_prev[p.y][p.x] >> 2), the shift arithmetic (the chain writes multiples of 4)
 *   merged_prev merged[f - 1] of the chain, int16 [H][W][2], 4-byte aligned
 *   centres     of block b, in this order: C0 = (0, 0); C1 = pred(b); C2 = merged_prev[yc][xc] >> 2, the co-located vector (what the
 *               chain's intra rule would assign); C3 .. C6 = pred(q) of the left, right, upper and lower neighbour block, each where it
 *               is in the grid AND its hop is usable
 *   candidates  the union (a vector proposed twice counts once) of centre + (ox, oy), |ox| <= r and |oy| <= r, r in 1 .. 3, whose displaced
 *               block lies inside the keyframe: 0 <= x0 + dx, x0 + w + dx <= W, 0 <= y0 + dy, y0 + h + dy <= H.  Nothing is padded or
 *               clamped.  (0, 0) always is one
 *   cost        SAD(cur block, key block at (dx, dy)) + lambda (|dx - C1x| + |dy - C1y|): the distance from the chain's own answer;
 *               lambda in 0 .. 255
 *   winner      the smallest cost; among equals the smallest dy, then the smallest dx.  (cost < 2^24 and
 *               (dy + 8192) 16384 + (dx + 8192) < 2^28: one 64-bit minimum of cost << 28 | that decides.)
 *   record      winner's SAD <= intra w h (intra in 0 .. 255): the block is ANCHORED, records_out[b] = (x0, y0, w, h, 4 dx, 4 dy, f - 1, 0).
 *               Otherwise records_out[b] = records_in[b], all eight fields.  f in 1 .. 16 (ref = f - 1 must stay below max_ref <= 16).
 *               f == 1: the hop already targets the keyframe; records_out = records_in, key and merged_prev are not read (merged_prev
 *               may be NULL), sad and stats are not touched
 *   sad         uint32 [by * bx], may be NULL; READ-MODIFY-WRITE: the entries of anchored blocks become the anchored SAD, the others
 *               are left as they were
 *   stats       int64 [ARSEG_BMA_NSTATS], 8-byte aligned, may be NULL; ACCUMULATED INTO: [0] anchored blocks, [1] anchored blocks whose
 *               hop was unusable (healed), [2] blocks kept on their hop, [3] sum over anchored blocks of |dx - C1x| + |dy - C1y| (the drift
 *               corrected, in pixels).  Integers: two runs are bit-equal
 *   records_out must not overlap records_in: neighbour centres read other blocks' input records while this block's output is written; in
 *               place the result would depend on scheduling.  Overlapping buffers are refused.
 * Enqueue only: one launch, no host synchronisation, no allocation, no workspace; a captured graph replays it.
 * ARSEG_EINVAL before any launch: a null cur, key, records_in or records_out; a null merged_prev at f >= 2; H or W outside 1 .. 8192; B
 * outside {8, 16}; r outside 1 .. 3; lambda or intra outside 0 .. 255; f outside 1 .. 16; a plane base that is not 4-byte aligned, a pitch
 * that is no multiple of 4 or below (W + 3) & ~3; records not 16-byte aligned, merged_prev or sad not 4-byte aligned, stats not 8-byte
 * aligned; overlapping record buffers.
 * Not covered: bidirectional chains, anchoring decoder records of arbitrary geometry, anchoring on a frame other than 0, choosing by cost
 * between hop and anchor (an anchor that passes the intra bound always wins), GOPs above 17 frames.  (The FLAGGED pixels of any chain --
 * bidirectional, decoder records of any geometry, any GOP length -- are healed by arseg_mv_chain_heal_fwd below.)
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_BMA_NSTATS 4
int arseg_block_motion_anchor_fwd(const uint8_t *cur, int64_t cur_pitch, const uint8_t *key, int64_t key_pitch, int H, int W, int B, int r, int lambda,
                                  int intra, int f, const int16_t *records_in, const int16_t *merged_prev, int16_t *records_out, uint32_t *sad,
                                  int64_t *stats, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Healing the flagged pixels of a motion chain on the keyframe (csrc/mv_chain_heal.hip).  A pixel that was intra or uncovered at one hop
 * stays flagged for the rest of the GOP and carries the substituted zero motion, although its content is usually visible again one frame
 * later and in the keyframe.  The anchor above mends that for the estimator's own records, before they are pushed.  This entry works on the
 * chain's OUTPUT instead: after the step entry of frame f, merged[f] and link[f] are dense planes whoever made the records, however they
 * were shaped and whichever step entry (P or bi) composed them.  The blocks of a fixed grid that hold flagged pixels are matched against
 * the keyframe, and where the flagged pixels match they get a direct one-hop vector to frame 0 and a clean link byte.  The chain's state
 * IS merged / link, so every later frame that composes through a healed pixel inherits the healed value.
 *   cur, key    luma8 byte planes [H][W] of frame f and of the keyframe; alignment and pitch exactly as arseg_block_motion_anchor_fwd: the
 *               base 4-byte aligned, the pitch a multiple of 4 and at least (W + 3) & ~3; the bytes of a row beyond W never count.
 *               H, W in 1 .. 8192
 *   merged_f    int16 [H][W][2], 4-byte aligned, IN PLACE: merged[f] as the step entry left it
 *   link_f      uint8 [H][W], IN PLACE: link[f] as the step entry left it
 *   blocks      B in {8, 16}: the grid of arseg_block_motion_fwd; block b = bi bx + bj, x0 = bj B, y0 = bi B, w = min(B, W - x0),
 *               h = min(B, H - y0)
 *   flagged     a pixel is FLAGGED iff (link_f[y][x] & flag_mask) != 0; flag_mask in 1 .. 7: which of ARSEG_LINK_INTRA / _UNCOVERED /
 *               _CLAMPED count.  n(b) = the number of flagged pixels of block b
 *   skipped     n(b) < min_flagged, min_flagged in 1 .. 64: nothing of the block is read further or written
 *   centres     of an examined block, in this order, with (xc, yc) = (x0 + w / 2, y0 + h / 2) by integer division and >> 2 an arithmetic
 *               shift: C0 = (0, 0); C1 = merged_f[yc][xc] >> 2, the chain's own answer, whether or not that pixel is flagged; C2 .. C5 =
 *               merged_f >> 2 at the centre pixel of the left, right, upper and lower neighbour block, each where the neighbour is in the
 *               grid AND that pixel is not flagged; C6 = merged_f >> 2 at the first unflagged pixel of the block itself in raster order, if
 *               there is one (the motion of the part of a split block the encoder did predict)
 *   candidates  the union (a vector proposed twice counts once) of centre + (ox, oy), |ox| <= r and |oy| <= r, r in 1 .. 3, whose displaced
 *               block lies inside the keyframe: 0 <= x0 + dx, x0 + w + dx <= W, 0 <= y0 + dy, y0 + h + dy <= H.  Nothing is padded or
 *               clamped.  (0, 0) always is one
 *   cost        SAD_all + lambda (|dx - C1x| + |dy - C1y|), SAD_all over all w h pixels of the block; lambda in 0 .. 255
 *   winner      the smallest cost; among equals the smallest dy, then the smallest dx (the anchor's 64-bit key,
 *               cost << 28 | (dy + 8192) << 14 | (dx + 8192))
 *   acceptance  SAD_flagged(winner) <= intra n(b), intra in 0 .. 255: SAD_flagged is the same sum restricted to the flagged pixels.  A
 *               cleared flag is a claim about those pixels only; it must not be bought by the unflagged rest of the block matching well.
 *               Where a whole block is flagged the two sums coincide
 *   result      every flagged pixel of an accepted (HEALED) block: merged_f[y][x] = (4 dx, 4 dy), link_f[y][x] = 0x10 (one hop, no
 *               flags).  Unflagged pixels and all pixels of other blocks keep every bit
 *   decisions   int16 [by * bx][8], 16-byte aligned, required: the hand-over between the two launches, and an output:
 *               (x0, y0, w, h, 4 dx, 4 dy, state, n(b)), state 0 healed, 1 examined and kept, 2 skipped; the vector is the winner for
 *               states 0 and 1 and zero for state 2
 *   sad         uint32 [by * bx], may be NULL: SAD_flagged(winner) of examined blocks; the entries of skipped blocks are untouched
 *   stats       int64 [ARSEG_HEAL_NSTATS], 8-byte aligned, may be NULL; ACCUMULATED INTO: [0] examined blocks, [1] healed blocks,
 *               [2] flagged pixels in examined blocks, [3] pixels healed, [4] flagged pixels in skipped blocks, [5] sum over healed blocks
 *               of |dx - C1x| + |dy - C1y|
 *   link_stats_row  int64 [ARSEG_LINK_NSTATS], 8-byte aligned, may be NULL: row f of the chain's counters, CORRECTED so that afterwards it
 *               equals what a recount of the new link_f would give: for every healed pixel its old flags and its old hop bin are
 *               subtracted and hop bin 1 is added
 * All integers: two runs are bit-equal.  Two launches on one stream (decide: a wave per block, writes decisions, sad and stats only, so no
 * block reads what another has healed; apply: rewrites the pixels).  Enqueue only: no workspace, no allocation, no host synchronisation;
 * a captured graph replays it.
 * ARSEG_EINVAL before any launch: a null cur, key, merged_f, link_f or decisions; H or W outside 1 .. 8192; B outside {8, 16}; r outside
 * 1 .. 3; lambda or intra outside 0 .. 255; flag_mask outside 1 .. 7; min_flagged outside 1 .. 64; a plane base that is not 4-byte aligned,
 * a pitch that is no multiple of 4 or below (W + 3) & ~3; merged_f not 4-byte aligned; decisions not 16-byte aligned; sad not 4-byte
 * aligned; stats or link_stats_row not 8-byte aligned.
 * Not covered: drift of UNFLAGGED pixels (the anchor's job, for estimated records), healing on a frame other than 0, blocks other than 8
 * and 16, chroma, sub-pel vectors.
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_HEAL_NSTATS 6
int arseg_mv_chain_heal_fwd(const uint8_t *cur, int64_t cur_pitch, const uint8_t *key, int64_t key_pitch, int H, int W, int B, int r, int lambda,
                            int intra, int flag_mask, int min_flagged, int16_t *merged_f, uint8_t *link_f, int16_t *decisions, uint32_t *sad,
                            int64_t *stats, int64_t *link_stats_row, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Quad-tree split of estimated block motion (csrc/block_motion_split.hip).  The estimators above give every 16 x 16 block one vector, so a
 * block that straddles the border of a moving object warps part of its pixels from the wrong place.  This entry searches the four 8 x 8
 * children of every 16 x 16 parent around the parent's and its neighbours' vectors and, where four vectors explain the block better than
 * one by more than split_gain, writes them as records of their own.  A caller pushes records_in || children as ONE list of 5 nb records to
 * arseg_mv_records_step_*: the children have the higher indices, so they win their pixels, and a row that was not split covers nothing.
 *   cur, ref    luma8 byte planes [H][W] of the current and of the reference frame; alignment and pitch exactly as
 *               arseg_block_motion_anchor_fwd: the base 4-byte aligned, the pitch a multiple of 4 and at least (W + 3) & ~3; the bytes of a
 *               row beyond W never count.  Level 0 of a luma pyramid and an aligned NV12 / I420 luma plane qualify.  H, W in 1 .. 8192
 *   parents     the B = 16 grid of arseg_block_motion_fwd: nb = by bx records in records_in, parent (bi, bj) is record b = bi bx + bj with
 *               x0 = 16 bj, y0 = 16 bi, w = min(16, W - x0), h = min(16, H - y0).  Of records_in only fields 4, 5 and 6 are read.  Parent
 *               b is USABLE iff field 6 == ref_index AND P(b) = round_half_even_div4 of fields 4 and 5 has |Px|, |Py| <= 500 AND the
 *               parent's block displaced by P lies inside the reference frame (0 <= x0 + Px, x0 + w + Px <= W, likewise y).  Every record
 *               the estimators above write that is not intra meets all three; hand-made records may not
 *   children    child q = 2 qy + qx of parent (bi, bj): x0 = 16 bj + 8 qx, y0 = 16 bi + 8 qy, w = min(8, W - x0), h = min(8, H - y0); it
 *               EXISTS iff w > 0 and h > 0
 *   centres     of an existing child, in this order: C0 = (0, 0); C1 = P(b), if b is usable; C2 = P of parent (bi, bj + (qx ? 1 : -1)), if
 *               that parent is in the grid and usable; C3 = P of parent (bi + (qy ? 1 : -1), bj), likewise
 *   candidates  the level-0 refinement's of arseg_block_motion_pyr_fwd: the union (a vector proposed twice counts once) of centre +
 *               (ox, oy), |ox| <= r and |oy| <= r, r in 1 .. 3, whose displaced child lies inside the reference frame.  Nothing is padded
 *               or clamped.  (0, 0) always is one, and so is P(b) of a usable parent
 *   cost        SAD + lambda (|dx| + |dy|), lambda in 0 .. 255
 *   winner      the smallest (cost, rank): rank(0, 0) = 0, otherwise rank = 1 + (dy + 511) 1023 + (dx + 511).  (|d| <= 503, so rank < 2^20
 *               and cost < 2^19: the refinement's 64-bit key.)  Per child: the winner (dx_q, dy_q), SAD_q, cost_q; for a usable parent
 *               also S_q(P), the child's SAD at the parent's vector.  A child is MATCHED iff SAD_q <= intra w h, intra in 0 .. 255
 *   decision    usable parent: split iff (sum_q S_q(P) + lambda (|Px| + |Py|)) - sum_q cost_q > split_gain, the sums over the existing
 *               children, the compare signed, split_gain in 0 .. 65535.  Four vectors pay lambda four times: the intended bias against
 *               splitting.  Unusable parent (intra): split iff at least one existing child is matched
 *   children    int16 [4 nb][8], 16-byte aligned; EVERY row is written every call, so the count is fixed for a captured graph.  Row
 *               4 b + q: split parent, existing and matched child: (x0, y0, w, h, 4 dx_q, 4 dy_q, ref_index, 0); split parent, existing
 *               child, not matched: (x0, y0, w, h, 0, 0, ARSEG_BM_INTRA_REF, 0); otherwise eight zeros (w = 0 covers nothing)
 *   child_sad   uint32 [4 nb], may be NULL: SAD_q of every existing child of every parent, split or not; 0 for a child that does not exist
 *   stats       int64 [ARSEG_BMS_NSTATS], 8-byte aligned, may be NULL; ACCUMULATED INTO: [0] parents split, [1] of those the unusable
 *               parents (healed), [2] child records written matched, [3] child records written intra, [4] sum of the decision's left-hand
 *               side over split usable parents, [5] pixels covered by matched children
 *   records_in  read only; children must not overlap it.  Overlapping buffers are refused.
 * All integers: two runs are bit-equal.  Enqueue only: one launch, no workspace, no allocation, no host synchronisation; a captured graph
 * replays it.
 * ARSEG_EINVAL before any launch: a null cur, ref, records_in or children; H or W outside 1 .. 8192; r outside 1 .. 3; lambda or intra
 * outside 0 .. 255; split_gain outside 0 .. 65535; ref_index outside 0 .. 15; a plane base that is not 4-byte aligned, a pitch that is no
 * multiple of 4 or below (W + 3) & ~3; records_in or children not 16-byte aligned, child_sad not 4-byte aligned, stats not 8-byte aligned;
 * overlapping record buffers.
 * Not covered: splitting below 8 x 8, and 16 x 8 / 8 x 16 partitions; splitting anchored records, or any use together with the keyframe
 * anchor; a split triggered by one child's error alone while the summed gain stays at or below split_gain; sub-pel vectors, chroma.
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_BMS_NSTATS 6
int arseg_block_motion_split_fwd(const uint8_t *cur, int64_t cur_pitch, const uint8_t *ref, int64_t ref_pitch, int H, int W, int r, int lambda,
                                 int intra, int split_gain, int ref_index, const int16_t *records_in, int16_t *children, uint32_t *child_sad,
                                 int64_t *stats, arseg_stream_t stream);
/* layout changes at the API boundary */
int arseg_nchw_to_nhwc_fwd(const float *in, float *out, int N, int C, int HW, int out_ld, arseg_stream_t stream);
int arseg_nhwc_to_nchw_fwd(const float *in, int in_ld, float *out, int N, int C, int HW, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 16-bit storage path (BASELINE configs[2]: BiSeNet-18 bf16, configs[4]: BiSeNet-18 0.3x fp16; model/bisenet.py:438-461,546-575).
 * Activations and weights are NHWC fp16 or bf16 (dtype = ARSEG_DT_F16 | ARSEG_DT_BF16), every product is ONE
 * v_mfma_f32_32x32x16_{f16,bf16}, accumulation and the epilogue (folded BN scale / bias, residual, activation) are fp32, results are
 * rounded to 16 bits once, at the store.  Cin % 8 == 0 (frames are ingested as NHWC8), in_ld / out_ld / res_ld % 8 == 0.
 *   arseg_pack_conv_weight16_host: OIHW fp32 -> [Cout][Kpad16] 16-bit with k = (r*S+s)*Cin_pad + ci, Kpad16 = arseg_packed_k16(...)
 *   arseg_conv2d16_fwd: desc as arseg_conv2d_fwd (tile_cfg: 0 auto; 1 / 2 = 64- / 128-channel tile with K step 32; 3 / 4 = the same with
 *                       K step 64; 5..8 = patch-resident kernel for 3x3 stride-1 pad == dil convs with Cin % 64 == 0 (the input patch of a
 *                       128- (5, 6) / 256-pixel (7, 8) tile stays in LDS for all nine taps, 64 / 128 output channels; no split-K;
 *                       ARSEG_EUNSUPPORTED for other shapes; 10..13 = the same kernel on squarer pixel tiles -- 10: 256 pixels as 8 x 32, 64 channels;
 *                       11: 16 x 16, 64 channels; 12: 8 x 32, 128 channels; 13: 128 pixels as 8 x 16, 64 channels -- refused on maps whose
 *                       default tile is already that narrow); 9 = stem kernel (7x7 stride 2 pad 3, NHWC8 -> 64 channels, no residual: all weights
 *                       resident in LDS, one staged input patch per 8x32 output tile); split_k: 0 = automatic -- K slices for launches whose tiles do not fill the chip, e.g. the 16x32-map
 *                       layers of BiSeNet-18 --, >= 1 explicit; deterministic: fp32 partial sums in `workspace`
 *                       (arseg_conv2d16_workspace_bytes(desc) bytes, 0 without split-K), summed in slice order by a second kernel that
 *                       applies the epilogue; split-K needs Cout % 8 == 0, otherwise one slice.  batch unused)
 *                       upsample2x = 1 (PSPUpsample): `in` is [N, H/2, W/2, in_ld], 3x3 stride-1 pad-1 dil-1, H and W even, Cin % 64 == 0,
 *                       patch plans 5..8 / 10..13 only (tile_cfg 0 = 7); every other plan and shape -> ARSEG_EUNSUPPORTED.  The patch is
 *                       interpolated from the low-resolution window while it is staged, with arseg_resize16_fwd's arithmetic and rounding:
 *                       the result equals arseg_resize16_fwd(2h x 2w, BILINEAR, align_corners 0) -> arseg_conv2d16_fwd, same plan, bit for bit.
 * ------------------------------------------------------------------------------------------- */
int arseg_packed_k16(int Cin_pad, int R, int S);
int arseg_pack_conv_weight16_host(const float *w_oihw_host, int Cout, int Cin, int R, int S, int Cin_pad, int dtype, void *out_host);
size_t arseg_conv2d16_workspace_bytes(const arseg_conv_desc *d);
int arseg_conv2d16_fwd(const arseg_conv_desc *d, int dtype, const void *in, const void *w_packed16, const float *scale,
                       const float *bias, const void *residual, void *out, void *workspace, size_t workspace_bytes,
                       arseg_stream_t stream);
/* The small layers on 16-bit NHWC tensors (C, ld % 8 == 0), same arithmetic as their fp32 counterparts above, fp32 inside:
 *   frame ingest: NCHW fp32 RGB -> NHWC8 (channels 3..7 zero) + bilinear align_corners=True downscale      evaluation.py:186-188
 *   maxpool 3x3 s2 p1; torch.mean(x,(2,3)) -> [N][C]; resize (nearest | bilinear, align_corners on / off); x*scale[n,c] (+add_full) (+add_vec[n,c])
 *   head: 1x1 classifier (fp32 weights) on a 16-bit feature -> fp32 NCHW logits (+ LogSoftmax)
 *   cast: fp32 <-> 16-bit element conversion (count % 8 == 0)
 *   warp_mvq16: arseg_warp_mvq_fwd on a 16-bit keyframe feature, fp32 C8 out (the CReFF kernels' input layout) */
int arseg_frame_to_nhwc8_16_fwd(const float *img, void *out, int dtype, int N, int H, int W, int h, int w, arseg_stream_t stream);
int arseg_maxpool3x3s2_16_fwd(const void *in, void *out, int dtype, int N, int H, int W, int C, arseg_stream_t stream);
size_t arseg_global_mean16_workspace_bytes(int N, int H, int W, int C);      /* fp32 partial sums of pixel slices */
int arseg_global_mean16_fwd(const void *in, int in_ld, void *out, int dtype, int N, int H, int W, int C, void *workspace,
                            size_t workspace_bytes, arseg_stream_t stream);
/* torch.amax(x,(2,3)) -> [N][C] in the storage dtype, exact (the result is one of the inputs; a NaN in a channel gives NaN); the workspace of
 * arseg_global_mean16_workspace_bytes.  PSPNet's auxiliary classifier input (model/pspnet.py:92-93). */
int arseg_global_max16_fwd(const void *in, int in_ld, void *out, int dtype, int N, int H, int W, int C, void *workspace,
                           size_t workspace_bytes, arseg_stream_t stream);
/* The folded PSP pyramid on the 16-bit path, twins of arseg_psp_pool_matrix_fwd / arseg_psp_prior_sum_fwd with the same limits and arithmetic:
 *   pool_matrix16: 16-bit NHWC in -> [N][rows][n_sizes * C] in the storage dtype (fp32 cell sums in the workspace, one rounding per element,
 *                  every element written, zeros included); workspace = arseg_psp_pool_matrix16_workspace_bytes (0: shape refused)
 *   prior_sum16:   t [N][rows][C] 16-bit (the prior 1x1 conv's output) -> [N,H,W,C] 16-bit sum of the levels' bilinear (align_corners=False)
 *                  upsamples, summed in fp32, rounded once (the residual of the bottleneck conv2d16, whose ReLU follows the add) */
size_t arseg_psp_pool_matrix16_workspace_bytes(int N, int H, int W, int C, int n_sizes, const int *sizes);
int arseg_psp_pool_matrix16_fwd(const void *in, int in_ld, void *out, int dtype, void *workspace, size_t workspace_bytes, int N, int H,
                                int W, int C, int n_sizes, const int *sizes, arseg_stream_t stream);
int arseg_psp_prior_sum16_fwd(const void *t, void *out, int dtype, int N, int H, int W, int C, int n_sizes, const int *sizes_host,
                              arseg_stream_t stream);
int arseg_resize16_fwd(const void *in, void *out, int dtype, int N, int C, int Hin, int Win, int Hout, int Wout, int mode,
                       int align_corners, int in_ld, int out_ld, arseg_stream_t stream);
int arseg_scale_add16_fwd(const void *x, const void *scale, const void *add_full, const void *add_vec, void *out, int dtype, int N,
                          int HW, int C, arseg_stream_t stream);
int arseg_head16_fwd(const void *p, int p_ld, int dtype, const float *wf, const float *bf, float *logits, int N, int HW, int C,
                     int n_cls, int log_softmax, arseg_stream_t stream);
int arseg_cast_fwd(const void *in, int in_dtype, void *out, int out_dtype, long long count, arseg_stream_t stream);
int arseg_warp_mvq16_fwd(const void *feature, int dtype, const int16_t *mv_q, float *out_c8, int N, int C, int Hp, int Wp, int H,
                         int W, arseg_stream_t stream);
/* The same with an explicit element stride between the frames' features: 0 = all N frames (the non-keyframes of one GOP) sample the same
 * keyframe feature -- one launch per GOP instead of one per frame. */
int arseg_warp_mvq16_shared_fwd(const void *feature, long long feat_n_stride, int dtype, const int16_t *mv_q, float *out_c8, int N, int C,
                                int Hp, int Wp, int H, int W, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluator tail                                                       evaluation.py:201-213
 * logits NCHW [N,n_cls,h,w] -> bilinear resize to HxW -> argmax -> pred int32 [N,H,W]
 * and hist[label*n_cls+pred] += 1 for label != ignore_label (hist: int64 [n_cls*n_cls], accumulated).
 * pred or hist/label may be NULL.
 *   align_corners != 0: the evaluator's F.interpolate(logits, label_size, align_corners=True) (evaluation.py:201);
 *   align_corners == 0: nn.Upsample(scale_factor, bilinear, align_corners=False) = BiSeNetOutput.up (model/bisenet.py:215-216),
 *                       i.e. head -> x8 upsample -> argmax without materialising the [n_cls,H,W] logits (the evaluator's own resize is
 *                       then the identity: labels have the frame's size).
 * argmax follows torch.argmax (first maximum wins; NaN counts as maximum).  The reference applies softmax first (evaluation.py:203):
 * monotone, so the result is the same except for top-two logits closer than fp32 exp() can separate (< 3e-8 apart, |logit| < 0.25).
 * ------------------------------------------------------------------------------------------- */
int arseg_argmax_confusion_fwd(const float *logits, const int64_t *label, int32_t *pred, int64_t *hist, int N,
                               int n_cls, int h, int w, int H, int W, int ignore_label, int align_corners, arseg_stream_t stream);

/* The same tail with one histogram per group of frames (the reference's result table is the mIoU per keyframe distance,
 * evaluation.py:272-303, 308-386): group = int32 [N] on the device, frame n counts into hist[group[n]]; hist: int64
 * [n_groups][n_cls*n_cls], accumulated.  A frame whose group id is outside [0, n_groups) gets its pred and counts nowhere.
 * pred is bit-equal to arseg_argmax_confusion_fwd's on the same input (same taps, blend order and argmax rule, both the per-pixel route
 * and the x2 / x4 / x8 align_corners == 0 run route).  pred or hist/label may be NULL; hist without group, n_groups < 1 and
 * n_cls > 32 are ARSEG_EINVAL. */
int arseg_argmax_confusion_grouped_fwd(const float *logits, const int64_t *label, const int32_t *group, int32_t *pred, int64_t *hist,
                                       int N, int n_groups, int n_cls, int h, int w, int H, int W, int ignore_label, int align_corners,
                                       arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Segmentation egress (csrc/egress.hip): head logits -> what a deployed segmenter hands on, in one launch for N frames, without an int32
 * or float frame-sized tensor in between.
 *   logits, N, n_cls, h, w, H, W, align_corners: as arseg_argmax_confusion_fwd.  Per output pixel the class k is EXACTLY what that entry point
 *               writes into pred for the same arguments (one device function serves both, csrc/arseg_device.h): the h == H && w == W route, the
 *               per-pixel bilinear route (either align_corners) and the x2 / x4 / x8 align_corners == 0 run route with its regrouped blend;
 *               first maximum wins, NaN counts as maximum.
 *   labels8     uint8 [N][H][W], labels_pitch bytes from row to row (>= W), labels_n_stride bytes from image to image (>= 0); value =
 *               lut ? lut[k] : k.  lut: HOST pointer to n_cls bytes (e.g. train id -> dataset label id), NULL = identity.  May be NULL.
 *   overlay     src0..2 -> dst0..2: the frame with the classes painted over it, source and destination in the same 8-bit `format`:
 *               ARSEG_SRC_RGB8 (plane 0), ARSEG_SRC_NV12 (planes 0, 1) or ARSEG_SRC_I420 (planes 0, 1, 2), planes, pitches and image strides
 *               as arseg_frame_ingest_fwd / arseg_frame_ingest_yuv_fwd take them, each side with its own.  Rows may be padded; nothing past a
 *               row's last sample is read or written.  dst0 NULL = no overlay (format and the plane arguments are then ignored).
 *   palette     HOST uint8 [n_cls][3], codes of the destination format: (R, G, B), or (Y, Cb, Cr) of the frame's colour matrix and range
 *   weights     HOST uint16 [n_cls], a_k in 0 .. 256: 0 leaves the frame's sample, 256 replaces it
 * Integer arithmetic, exact:
 *   RGB8, per channel c:     dst = (src (256 - a_k) + P[k][c] a_k + 128) >> 8
 *   4:2:0 luma, per pixel:   Y'  = (Y (256 - a_k) + P[k][0] a_k + 128) >> 8
 *   4:2:0 chroma, per sample, over the four luma pixels i of its 2 x 2 block with classes k_i:  A = sum a_{k_i},
 *                            C'  = (C (1024 - A) + sum a_{k_i} P[k_i][c] + 512) >> 10          c = 1 (Cb), 2 (Cr)
 *   (equal weights: the 2 x 2 box average of the painted colour, the chroma model of a 4:2:0 encoder's input)
 * In place: every destination sample is read from the source and written by the same thread exactly once, so a destination plane may BE its
 * source plane (same pointer, pitch and image stride), or be entirely distinct from every source plane.  Partial overlap is undefined.
 * labels8 must not overlap any other buffer.
 * Enqueue only: no allocation, no synchronisation.  ARSEG_EINVAL, before any launch: null logits; labels8 and dst0 both null; dst0 without
 * src0, palette or weights (or without the format's further planes on either side); n_cls < 1 or > 32; a weight above 256; a non-positive
 * size; odd H or W with NV12 / I420; a pitch smaller than a row; a negative image stride; a format other than the three above (P010 / I010
 * are rejected).
 * Not covered: 10-bit, 4:2:2 or 4:4:4 destinations; text or legends; the encoder; the confusion histogram (evaluation keeps
 * arseg_argmax_confusion_fwd).  (The outlines of the mask's regions as polygons, for a vector overlay: arseg_rle_contours_fwd, below.)
 * ------------------------------------------------------------------------------------------- */
int arseg_segment_egress_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners, const uint8_t *lut,
                             uint8_t *labels8, int64_t labels_pitch, int64_t labels_n_stride, int format, const void *src0, const void *src1,
                             const void *src2, int64_t src_pitch0, int64_t src_pitch1, int64_t src_pitch2, int64_t src_n_stride0,
                             int64_t src_n_stride1, int64_t src_n_stride2, void *dst0, void *dst1, void *dst2, int64_t dst_pitch0,
                             int64_t dst_pitch1, int64_t dst_pitch2, int64_t dst_n_stride0, int64_t dst_n_stride1, int64_t dst_n_stride2,
                             const uint8_t *palette, const uint16_t *weights, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Segmentation confidence (csrc/confidence.hip): head logits -> how much to trust each pixel and each frame, in one launch for N frames and
 * one pass over the logits, without probabilities or any other float frame-sized tensor in between.  The online signal of a stream without
 * ground truth: the softmax's top-1 probability per output pixel, its sum over the frame and the number of uncertain pixels.
 *   logits, N, n_cls, h, w, H, W, align_corners: as arseg_argmax_confusion_fwd and arseg_segment_egress_fwd, with their route choice (h == H
 *               && w == W; per-pixel bilinear, either align_corners; the x2 / x4 / x8 align_corners == 0 run route with its regrouped blend).
 *               The blended class values v_k of an output pixel and its class k* are those of the one label rule (csrc/arseg_device.h): k* is
 *               EXACTLY what arseg_argmax_confusion_fwd writes into pred for the same arguments (first maximum wins, NaN counts as maximum).
 *   per pixel   m = max_k v_k, Z = sum_k exp(v_k - m) in fp32 (one pass over the classes: running maximum, rescaled sum);
 *               p1 = 1 / Z;  p2 = exp(v_second - m) / Z, v_second the largest value over k != k* (p2 = 0 for n_cls == 1).
 *               softmax(log_softmax(x)) = softmax(x): log-probability outputs need no special case.
 *   kind        enum arseg_conf_kind: ARSEG_CONF_TOP1 c = p1;  ARSEG_CONF_MARGIN c = p1 - p2
 *   code        q = (uint8) floor(255 c + 0.5), never above 255; a pixel whose c is NaN (a NaN logit, a +inf maximum, all classes -inf)
 *               gets q = 0
 * Outputs, any non-empty subset (NULL = not wanted):
 *   conf8       uint8 [N][H][W] of q, conf_pitch bytes from row to row (>= W), conf_n_stride bytes from image to image (>= 0); nothing past
 *               a row's last sample is written
 *   labels8     uint8 [N][H][W], labels_pitch / labels_n_stride alike; value = lut ? lut[k*] : k*.  lut: HOST pointer to n_cls bytes, NULL =
 *               identity (as in arseg_segment_egress_fwd)
 *   stats       int64 [N][ARSEG_CONF_NSTATS] on the device, ACCUMULATED INTO (like hist); for frame n
 *                 stats[n][0]     += sum of q over the frame
 *                 stats[n][1]     += number of pixels with q < low (low: 0 .. 256)
 *                 stats[n][2 + k] += number of pixels with k* == k (not mapped through lut), k < n_cls; entries from 2 + n_cls on are untouched
 *               Integer sums: independent of the order of the atomic adds, so two runs are bit-equal.  stats alone equals the stats of the
 *               same call with planes.
 * The output buffers must not overlap each other or the logits.
 * Enqueue only: no allocation, no synchronisation.  ARSEG_EINVAL, before any launch: null logits; conf8, labels8 and stats all null;
 * n_cls < 1 or > 32; a non-positive size; a pitch smaller than W; a negative image stride; an unknown kind; low outside 0 .. 256.
 * Not covered: entropy or calibrated confidences, per-class confidence, confidence painted into overlays, 10-bit planes.
 * ------------------------------------------------------------------------------------------- */
enum arseg_conf_kind { ARSEG_CONF_TOP1 = 0, ARSEG_CONF_MARGIN = 1 };
#define ARSEG_CONF_NSTATS (2 + 32)
int arseg_segment_confidence_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners, int kind, int low,
                                 const uint8_t *lut, uint8_t *conf8, int64_t conf_pitch, int64_t conf_n_stride, uint8_t *labels8,
                                 int64_t labels_pitch, int64_t labels_n_stride, int64_t *stats, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal consistency (csrc/consistency.hip): does the mask of a frame agree with the mask of a reference frame -- the GOP's keyframe --
 * fetched through the motion between them?  The label-free signal the confidence cannot give: a drifted chain or a scene cut inside a GOP
 * can still produce sharp softmaxes.  One launch for N frames and one pass over the logits; no int32 labels and no resized logits exist.
 *   logits, N, n_cls, h, w, H, W, align_corners, lut, pitches and image strides: exactly as arseg_segment_confidence_fwd takes them, with its
 *               route choice (h == H && w == W; per-pixel bilinear, either align_corners; the x2 / x4 / x8 align_corners == 0 run route).
 *               The class k* of a pixel is the one label rule (csrc/arseg_device.h): EXACTLY what arseg_argmax_confusion_fwd writes into pred.
 *   ref_labels  uint8 [R][H][W] on the device, TRAIN IDS (not mapped through lut), ref_pitch bytes from row to row (>= W), ref_image_stride
 *               bytes from image to image; ref_image_stride == 0: one plane shared by all N frames (the keyframe).  A value >= n_cls is void
 *               (e.g. 255).
 *   mv_q        int16 [N][H][W][2] on the device, contiguous, 4-byte aligned: (mvx, mvy) in quarter pels accumulated back to the reference
 *               frame, sign and units of arseg_merge_motion_fwd's output.  Target of pixel (x, y):
 *                 tx = x + round_half_even_div4(mvx)      ty = y + round_half_even_div4(mvy)
 *               (np.round(v / 4): halves go to the even neighbour, the rounding of mergeMotion).  NO clamp.
 *   per pixel   exactly one of four outcomes, decided in this order:
 *                 outside  (tx, ty) is not in [0, W) x [0, H); the reference plane is not read
 *                 void     ref_labels[ty][tx] >= n_cls (plane form: or the source label >= n_cls)
 *                 agree    ref_labels[ty][tx] == k*
 *                 differ   otherwise
 * Outputs, any non-empty subset (NULL = not wanted):
 *   labels_out  uint8 [N][H][W], labels_pitch / labels_image_stride in bytes; value = lut ? lut[k*] : k* (lut: HOST pointer to n_cls bytes)
 *   change_out  uint8 [N][H][W], change_pitch / change_image_stride alike: 0 agree, 255 differ, 128 not compared (outside or void); nothing
 *               past a row's last sample is written
 *   stats       int64 [N][ARSEG_TC_NSTATS] on the device, ACCUMULATED INTO (like hist and the confidence statistics); for frame n
 *                 stats[n][0]      += compared pixels (agree + differ)
 *                 stats[n][1]      += outside pixels
 *                 stats[n][2]      += void pixels
 *                 stats[n][3 + k]  += compared pixels with k* == k            (cur_k)
 *                 stats[n][35 + k] += compared pixels with ref == k           (ref_k)
 *                 stats[n][67 + k] += compared pixels with k* == ref == k     (inter_k)         k < n_cls; the other entries are untouched
 *               Integers: independent of the order of the atomic adds, so two runs are bit-equal; stats alone equals the stats of the same
 *               call with planes.  Agreement rate of a frame = sum_k inter_k / compared; temporal consistency in the mIoU form = the mean
 *               over the classes with cur_k + ref_k - inter_k > 0 of inter_k / (cur_k + ref_k - inter_k).
 * arseg_labels_consistency_fwd is the plane form: the same comparison and the same counters with an 8-bit TRAIN-ID plane labels_in (uint8
 * [N][H][W], in_pitch / in_image_stride in bytes) as the source instead of logits; a source label >= n_cls makes an inside pixel void.  For
 * callers that hold labels8 planes already, or that compare consecutive frames with a per-frame field of their own (R = N).
 * The output buffers must not overlap each other or any input.
 * Enqueue only: no allocation, no synchronisation.  ARSEG_EINVAL, before any launch: null logits / labels_in; null ref_labels or mv_q; an
 * mv_q that is not 4-byte aligned; no output at all; n_cls < 1 or > 32; a non-positive size; a pitch smaller than W; a negative image
 * stride.  (The tail refuses no shape on the run route -- a shape that is not an exact x2 / x4 / x8 takes the per-pixel route -- so neither
 * does this.)
 * arseg_labels_consistency_linked_fwd is the plane form gated by the chain's link bytes (arseg_mv_records_step_link_fwd above), four more
 * arguments:
 *   link        uint8 [N][H][W] on the device, link_pitch bytes from row to row (>= W), link_image_stride bytes from frame to frame: the
 *               link plane of each frame
 *   link_mask   the flags that gate (ARSEG_LINK_INTRA | ARSEG_LINK_UNCOVERED | ARSEG_LINK_CLAMPED, any subset; the hop bits may be named too)
 *   unlinked    int64 [N] on the device, ACCUMULATED INTO, may be NULL
 * A pixel with link & link_mask != 0 takes a fifth outcome, UNLINKED, decided FIRST: neither mv_q nor the reference is read for it,
 * change_out is 128, it enters no counter of stats, and unlinked[n] is incremented.  Otherwise the four outcomes above in their order.  The
 * stats layout is unchanged; for every frame compared + outside + void + unlinked = H W.  link_mask == 0 gives the outputs of
 * arseg_labels_consistency_fwd bit for bit.  ARSEG_EINVAL additionally: a null link, link_pitch < W, a negative link_image_stride, an unlinked
 * that is not 8-byte aligned.
 * Not covered: sub-pixel comparison of label probabilities, occlusion reasoning beyond the link flags (the logits form has no linked
 * variant), consecutive-frame fields (the plane form takes one).
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_TC_NSTATS (3 + 3 * 32)
int arseg_segment_consistency_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners,
                                  const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                  const uint8_t *lut, uint8_t *labels_out, int64_t labels_pitch, int64_t labels_image_stride,
                                  uint8_t *change_out, int64_t change_pitch, int64_t change_image_stride, int64_t *stats,
                                  arseg_stream_t stream);
int arseg_labels_consistency_fwd(const uint8_t *labels_in, int64_t in_pitch, int64_t in_image_stride, int N, int n_cls, int H, int W,
                                 const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                 uint8_t *change_out, int64_t change_pitch, int64_t change_image_stride, int64_t *stats,
                                 arseg_stream_t stream);
int arseg_labels_consistency_linked_fwd(const uint8_t *labels_in, int64_t in_pitch, int64_t in_image_stride, int N, int n_cls, int H, int W,
                                        const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                        uint8_t *change_out, int64_t change_pitch, int64_t change_image_stride, int64_t *stats,
                                        const uint8_t *link, int64_t link_pitch, int64_t link_image_stride, uint8_t link_mask,
                                        int64_t *unlinked, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The keyframe prior along the motion chain (csrc/stabilise.hip): the actuator for what the consistency counters measure.  Where the motion
 * link of a pixel is trustworthy and the frame's own decision is marginal, the pixel keeps the class the keyframe had at the
 * motion-compensated position.  One launch for N frames and one pass over the logits; the output is an ordinary labels8 plane.
 *   logits, N, n_cls, h, w, H, W, align_corners, lut, pitches and image strides; ref_labels, ref_pitch, ref_image_stride (0: one plane for all
 *               N frames); mv_q: exactly as arseg_segment_consistency_fwd takes them, with its three routes and its route choice (that of
 *               arseg_argmax_confusion_fwd).  k*, m = v_{k*} and the blended class values v_k of a pixel are those of the one label rule
 *               (csrc/arseg_device.h).  Target of pixel (x, y): tx = x + round_half_even_div4(mvx), ty = y + round_half_even_div4(mvy), NO clamp.
 *   bonus       fp32 [N] ON THE DEVICE, 4-byte aligned: the hold threshold beta_n of frame n in logit units (on the device so that a captured
 *               graph can be replayed with new values)
 *   link, link_pitch, link_image_stride, link_mask: as in arseg_labels_consistency_linked_fwd; link == NULL or link_mask == 0 turns the gate off
 *   ref_conf    uint8 confidence codes of the reference (arseg_segment_confidence_fwd's conf8 of the keyframe), conf_pitch / conf_image_stride
 *               with the conventions of ref_labels (stride 0: one plane for all N frames); NULL turns the gate off
 *   ref_low     0 .. 256: a pixel whose reference code, read at the same target, is < ref_low offers no prior (0: no pixel)
 *   per pixel   exactly one of seven outcomes, decided in this order:
 *                 0 UNLINKED  link & link_mask != 0; neither mv_q nor the reference is read
 *                 1 OUTSIDE   (tx, ty) is not in [0, W) x [0, H); the reference planes are not read
 *                 2 VOID      c_ref = ref_labels[ty][tx] >= n_cls
 *                 3 WEAK      ref_conf[ty][tx] < ref_low
 *                 4 AGREE     c_ref == k*
 *                 5 HELD      m - v_{c_ref} < beta_n: strict, in fp32, false when an operand is NaN (a NaN logit, -inf - -inf, a NaN beta);
 *                             so beta <= 0 holds nothing, and n_cls == 1 never holds
 *                 6 OWN       otherwise
 *               The label of the pixel is c_ref for HELD and k* otherwise.
 * Outputs, any non-empty subset (NULL = not wanted):
 *   labels_out  uint8 [N][H][W], labels_pitch / labels_image_stride in bytes; value = lut ? lut[label] : label (lut: HOST pointer to n_cls bytes)
 *   hold_out    uint8 [N][H][W], hold_pitch / hold_image_stride alike: 0 AGREE, 255 HELD, 192 OWN, 128 for the outcomes 0 .. 3; nothing past
 *               a row's last sample is written
 *   stats       int64 [N][ARSEG_ST_NSTATS] on the device, ACCUMULATED INTO; for frame n
 *                 stats[n][o]      += pixels with outcome o, o = 0 .. 6 (they sum to H W per launch); stats[n][7] is reserved and untouched
 *                 stats[n][8 + k]  += HELD pixels with c_ref == k     (into_k)
 *                 stats[n][40 + k] += HELD pixels with k* == k        (from_k)           k < n_cls; the other entries are untouched
 *               Integers: independent of the order of the atomic adds, so two runs are bit-equal; stats alone equals the stats of the same
 *               call with planes.  With the same gates, AGREE + HELD is the agreeing count arseg_labels_consistency_linked_fwd finds on
 *               labels_out: agreement along the chain can only rise.
 * The output buffers must not overlap each other or any input.
 * Enqueue only: no allocation, no synchronisation.  ARSEG_EINVAL, before any launch: everything arseg_segment_consistency_fwd refuses (with
 * hold_out in the place of change_out); a null or misaligned bonus; ref_low outside 0 .. 256; with a link, link_pitch < W or a negative
 * link_image_stride; with a ref_conf, conf_pitch < W or a negative conf_image_stride.
 * Not covered: a plane form (without logits there is no margin), consecutive-frame recurrence (the chain holds motion to the keyframe only).
 * (A backward-compatible addition: ARSEG_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_ST_NSTATS (8 + 2 * 32)
int arseg_segment_stabilise_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners,
                                const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                const float *bonus, const uint8_t *link, int64_t link_pitch, int64_t link_image_stride, uint8_t link_mask,
                                const uint8_t *ref_conf, int64_t conf_pitch, int64_t conf_image_stride, int ref_low,
                                const uint8_t *lut, uint8_t *labels_out, int64_t labels_pitch, int64_t labels_image_stride,
                                uint8_t *hold_out, int64_t hold_pitch, int64_t hold_image_stride, int64_t *stats, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Run-length coded label planes (csrc/rle.hip): the 8-bit planes above (labels8, change8, conf8) are a few thousand constant runs per
 * frame, and what leaves the GPU for a bus, a database or a browser is run-length codes.  Encoded and decoded on the device, without a host
 * synchronisation, so both calls can be captured in a HIP graph.
 * Row-run format.  Runs never cross a row.  In row y of frame n a run begins at x = 0 and at every x >= 1 with plane[y][x] != plane[y][x-1].
 *   row_start   int32 [N][H+1] on the device, contiguous, 4-byte aligned, OVERWRITTEN (not accumulated into):
 *                 row_start[n][y] = number of runs in rows 0 .. y-1 of frame n;  row_start[n][0] = 0;
 *                 row_start[n][H] = the number of runs the frame needs -- always exact, whatever cap is.
 *   runs        uint32 [N][cap] on the device, 4-byte aligned.  Run i of frame n, in (y, x) order, is the word (x_first << 8) | value; value
 *               is the plane's byte: any byte 0 .. 255 is legal, there is no n_cls.  A run ends where the next run of its row starts, or at W.
 *               Overflow: a word whose index is >= cap is not written; every word below cap is written and exact; nothing at or past
 *               runs[n][cap] is touched.  The caller detects overflow as row_start[n][H] > cap.
 *               runs == NULL: cap is ignored and row_start alone is produced (the sizing pass).
 * arseg_labels_rle_fwd: labels uint8 [N][H][W] on the device, pitch bytes from row to row (>= W, any parity), image_stride bytes from image
 *   to image (>= 0).  Three launches (count per row, a prefix per frame, emit; the per-row counts live in row_start[n][y+1] in between); no
 *   workgroup waits for another.  Enqueue only: no allocation, no synchronisation, no workspace.
 * arseg_rle_decode_fwd: the inverse, for a receiving GPU and for round trips.  Every pixel covered by a stored run gets that run's value;
 *   the pixels of runs with an index >= cap are left untouched; nothing past a row's last sample is written.  The last stored run of an
 *   overflowed frame, when the next run of its row was cut off, has no stored end: its first pixel is written and no more.
 *   Undefined results if row_start is not non-decreasing with row_start[n][0] == 0; even then nothing outside runs[n][0 .. cap) is read and
 *   nothing outside the rows is written.
 * The buffers must not overlap.
 * ARSEG_EINVAL, before any launch: null labels / labels_out or row_start (decode: null runs); a row_start or runs that is not 4-byte aligned;
 * cap < 0 with non-null runs; non-positive N, H or W; pitch < W; a negative image stride; W > 1 << 24 (x_first has 24 bits); H * W > INT32_MAX.
 * Not covered: COCO's column-major per-class RLE; entropy coding; runs across rows; the run count fused into the tail kernels (the tail
 * writes labels8 as before and the encoder reads that plane).
 * ------------------------------------------------------------------------------------------- */
int arseg_labels_rle_fwd(const uint8_t *labels, int64_t pitch, int64_t image_stride, int N, int H, int W, int32_t *row_start, uint32_t *runs,
                         int64_t cap, arseg_stream_t stream);
int arseg_rle_decode_fwd(const int32_t *row_start, const uint32_t *runs, int64_t cap, int N, int H, int W, uint8_t *labels_out, int64_t pitch,
                         int64_t image_stride, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Connected regions of a run code (csrc/regions.hip): for every connected region of one value its value, area, bounding box and the sums
 * that give its centroid -- what a tracker, an alerting rule or a click target starts from -- labelled on the device from the runs alone
 * (a union-find over a few thousand runs; the plane is not read), without a host synchronisation: capturable in a HIP graph behind
 * arseg_labels_rle_fwd.
 * Input: row_start int32 [N][H+1] and runs uint32 [N][cap] exactly as arseg_labels_rle_fwd writes them, the same N, H, W and cap;
 *   connectivity 4 or 8.
 * Adjacency.  Run i of row y covers [a0, a1) (a1: the start of the next run of its row, or W) and has value v; run j of row y-1 covers
 *   [b0, b1) and has the same value.  4-connectivity: adjacent iff a0 < b1 && b0 < a1.  8-connectivity: adjacent iff a0 < b1 + 1 &&
 *   b0 < a1 + 1.  Runs of one row are never adjacent (neighbours in a row differ by construction).  A region is a connected component of
 *   this graph.  Every byte value forms regions: there is no background class and no n_cls.
 * Order.  A region's root is its run with the smallest index in the frame's (y, x) order; regions are numbered 0 .. R-1 by rising root
 *   index (the raster order of each region's first pixel).  Every output is a pure function of the input, whatever the order of the merges.
 * Outputs, all integers, all OVERWRITTEN:
 *   n_regions   int32 [N]: R of the frame, exact whatever cap and rcap are.
 *   run_region  int32 [N][cap]: the region number of each stored run; the words from row_start[n][H] up to cap are untouched.  Exact also
 *               when R > rcap.
 *   regions     int64 [N][rcap][8], 8-byte aligned: per region {value, area, x_min, y_min, x_max, y_max, sum_x, sum_y}; the bounds are
 *               inclusive pixel coordinates, sum_x and sum_y sums over the region's pixels (centroid = sum / area).  A run [a0, a1) of row y
 *               gives area += a1 - a0, sum_x += (a0 + a1 - 1)(a1 - a0) / 2, sum_y += y (a1 - a0).  The rows below min(R, rcap) are exact,
 *               the rows from min(R, rcap) on are untouched; the caller detects the overflow as R > rcap.  regions == NULL with rcap == 0:
 *               the sizing and labelling pass.
 * A frame whose run code overflowed (row_start[n][H] > cap) has an incomplete graph: n_regions[n] = -1, and neither run_region[n] nor
 *   regions[n] is touched.  Decided on the device; nothing comes to the host.
 * workspace: the caller's, 4-byte aligned, >= arseg_rle_regions_workspace_bytes(N, cap) bytes (else ARSEG_EWORKSPACE): the forest, one
 *   int32 parent per run slot.  Its contents are scratch.
 * Five launches (init, link, flatten, number, relabel + accumulate); no workgroup waits for another.  Enqueue only: no allocation, no
 *   synchronisation.  The buffers must not overlap.
 * A malformed run code (a row_start that does not rise, x_first out of order or >= W) gives undefined regions, but nothing outside the
 *   caller's buffers is read or written: indices and columns are clamped, and every loop that follows a parent pointer is bounded, since
 *   parents only ever point to smaller indices.
 * ARSEG_EINVAL, before any launch: null row_start, runs, n_regions or run_region; one of them or the workspace not 4-byte aligned, regions
 *   not 8-byte aligned; non-positive N, H or W; cap <= 0; rcap < 0; regions == NULL with rcap > 0; connectivity other than 4 or 8;
 *   W > 1 << 24; H * W > INT32_MAX; a null workspace.
 * Not covered: a dense 32-bit instance-id plane; regions across frames; the labelling fused into the run coder.
 *   (Which region of another frame a region came from: arseg_region_links_fwd, below.  Removing or merging small regions:
 *   arseg_rle_absorb_fwd, below.  The regions' outlines as polygons: arseg_rle_contours_fwd, below.)
 * ------------------------------------------------------------------------------------------- */
size_t arseg_rle_regions_workspace_bytes(int N, int64_t cap);
int arseg_rle_regions_fwd(const int32_t *row_start, const uint32_t *runs, int64_t cap, int N, int H, int W, int connectivity,
                          int32_t *n_regions, int32_t *run_region, int64_t *regions, int64_t rcap, void *workspace, size_t workspace_bytes,
                          arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Links between the regions of two frames along the motion chain (csrc/links.hip): for every region of a frame, which region of a
 * reference frame -- the GOP's keyframe -- it came from, and how much of it; the object-level form of arseg_segment_consistency_fwd.
 * Computed on the device from the two run codes, their run_region and the motion field, without a host synchronisation: capturable in a
 * HIP graph behind arseg_rle_regions_fwd.  mv_q is the only input of the size of a frame.
 * Input.  The CURRENT frames: row_start int32 [N][H+1], runs uint32 [N][cap], n_regions int32 [N] and run_region int32 [N][cap] exactly as
 *   arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them.  The REFERENCE frames: the same four arrays with their own ref_cap;
 *   ref_shared = 1: one reference frame for all N (the keyframe), ref_shared = 0: one per current frame (consecutive-frame use with a field
 *   of the caller's own).  mv_q int16 [N][H][W][2], contiguous, 4-byte aligned, sign and units of arseg_segment_consistency_fwd; NULL = zero
 *   motion.
 * Per pixel.  Pixel (x, y) of current frame n lies in run i with value v and region r = run_region[n][i].  Its target is
 *     tx = x + round_half_even_div4(mvx)      ty = y + round_half_even_div4(mvy)          (no clamp, as arseg_segment_consistency_fwd)
 *   (tx, ty) not in [0, W) x [0, H): the pixel is OUTSIDE.  Otherwise the reference run j that covers tx in row ty has value u and region k:
 *   u == v: the pixel counts 1 into the pair (r, k); u != v: it counts nothing (per region: area - outside - same such pixels).
 * Outputs, all integers, all OVERWRITTEN, every one a pure function of the inputs whatever the order of the atomics:
 *   n_pairs     int32 [N]: the number of distinct pairs (r, k) with a count > 0; or
 *                 -1  the frame cannot be linked: its run code or its reference's overflowed (row_start[.][H] > cap), or either n_regions
 *                     entry is negative.  Nothing else of that frame is touched.
 *                 -2  more than pcap distinct pairs.  Nothing else of that frame is touched; the caller retries with a larger table.
 *   links       int64 [N][rcap][6], 8-byte aligned: per current region r {ref_region, overlap, same, outside, mutual, n_ref}.
 *                 ref_region  the k with the largest pair count, ties to the smaller k; -1 if none
 *                 overlap     that pair's count                    same     the sum of r's pair counts
 *                 outside     as defined above                     n_ref    the number of distinct k
 *                 mutual      1 iff back[ref_region].cur_region == r (exact whatever kcap is, also with back == NULL)
 *               The rows below min(R, rcap) are exact, the rows from there on are untouched.  links == NULL with rcap == 0: not wanted.
 *   back        int64 [N][kcap][4], 8-byte aligned: per reference region k and current frame {cur_region, overlap, covered, n_cur}:
 *               cur_region the r with the largest count (ties to the smaller r, -1 if none), overlap that count, covered the sum over r of
 *               the pair counts, n_cur the number of distinct r.  Exact below min(R_ref, kcap), untouched above.  back == NULL with
 *               kcap == 0: not wanted.
 * workspace: the caller's, 8-byte aligned, >= arseg_region_links_workspace_bytes(N, pcap) bytes (else ARSEG_EWORKSPACE): per frame an open
 *   addressed table of pcap slots for the pairs (a 64-bit key and a 64-bit count), one of pcap slots for the best current region of every
 *   reference region, and a flag.  pcap: any value >= 1.  Probing visits every slot before it gives up, so an insert fails if and only if
 *   the frame has more than pcap distinct pairs: -2 does not depend on timing.  Its contents are scratch.
 * Six launches (clear, vote, rows, outside -- not without mv_q or links --, resolve, finish); no workgroup waits for another.  Enqueue only:
 *   no allocation, no synchronisation.  The buffers must not overlap.
 * Malformed input (a run_region outside [0, R), a row_start that does not rise, x_first out of order) gives meaningless links, but nothing
 *   outside the caller's buffers is read or written: indices and columns are clamped as arseg_rle_regions_fwd clamps them, and every loop
 *   is bounded.
 * ARSEG_EINVAL, before any launch: a null row_start, runs, n_regions or run_region of either side, or a null n_pairs; one of them or mv_q
 *   not 4-byte aligned; links, back or the workspace not 8-byte aligned; non-positive N, H, W, cap, ref_cap or pcap; negative rcap or kcap;
 *   links == NULL with rcap > 0, back == NULL with kcap > 0; ref_shared other than 0 or 1; W > 1 << 24; H * W > INT32_MAX; a null
 *   workspace.
 * Not covered: frame-to-frame motion fields (the caller supplies one with ref_shared = 0); occlusion reasoning; appearance features;
 *   many-to-many assignment; thresholds of any kind (what counts as the same object is the caller's decision).
 * ------------------------------------------------------------------------------------------- */
size_t arseg_region_links_workspace_bytes(int N, int64_t pcap);
int arseg_region_links_fwd(const int32_t *row_start, const uint32_t *runs, const int32_t *n_regions, const int32_t *run_region, int64_t cap,
                           const int32_t *ref_row_start, const uint32_t *ref_runs, const int32_t *ref_n_regions,
                           const int32_t *ref_run_region, int64_t ref_cap, int ref_shared, const int16_t *mv_q, int N, int H, int W,
                           int32_t *n_pairs, int64_t *links, int64_t rcap, int64_t *back, int64_t kcap, int64_t pcap, void *workspace,
                           size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Small regions absorbed into their neighbours (csrc/absorb.hip): the specks of a mask -- few-pixel islands of another class along object
 * borders and where the motion field tears -- take the value of the neighbour they share the longest border with, on the run code (a few
 * thousand words per frame, not the plane) and on the device, without a host synchronisation: capturable in a HIP graph behind
 * arseg_rle_regions_fwd.
 * Input: row_start int32 [N][H+1], runs uint32 [N][cap], n_regions int32 [N], run_region int32 [N][cap] and regions int64 [N][rcap][8]
 *   exactly as arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them (either connectivity); the same N, H, W; min_area >= 1; protect: a
 *   host table of 256 bytes or NULL, read during the call and handed to the kernels by value, as lut is.
 * Definitions, all integer.  Region r is PROTECTED iff protect && protect[value_r]; STABLE iff area_r >= min_area or it is protected; SMALL
 *   otherwise.  border(r, s), r != s: the number of 4-neighbour pixel pairs (p, q) with p in r and q in s, whatever connectivity the
 *   regions were labelled with.  In runs: two consecutive runs of one row add 1 to the pair of their regions; run i of row y over [a0, a1)
 *   and run j of row y-1 over [b0, b1) of different regions add min(a1, b1) - max(a0, b0) when that is positive.
 *   target(r) of a small r: the stable s with the largest border(r, s), ties to the smaller s.  A small region without a stable neighbour
 *   has no target and stays as it is.  One pass, no cascade: every decision reads the input only, so the result does not depend on timing;
 *   a caller who wants a second pass labels the output and calls again.
 *   The new value of a run: value_target(r) if its region r is small and has a target, its own value otherwise.
 * Outputs, all integers, all OVERWRITTEN:
 *   out_row_start int32 [N][H+1], out_runs uint32 [N][out_cap]: the row-run code of the resulting plane, word for word what
 *               arseg_labels_rle_fwd writes for the decoded, re-valued plane: neighbouring runs of a row whose new values are equal are
 *               one run.  The encoder's overflow rule: out_row_start[n][H] is always exact, a word whose index is >= out_cap is not
 *               written, nothing at or past out_runs[n][out_cap] is touched.  The output never needs more runs than the input:
 *               out_cap = cap cannot overflow.
 *   target      int32 [N][tcap]: per region below min(R, tcap) -1: stable, -2: small and left alone, else the s it was absorbed into; the
 *               rows from there on are untouched.  target == NULL with tcap == 0: not wanted.
 *   n_absorbed  int32 [N]: the number of regions with a target; or
 *                 -1  the frame cannot be processed: row_start[n][H] > cap, n_regions[n] < 0, or n_regions[n] > rcap (the area of every
 *                     region is needed).  Nothing else of that frame is touched, out_row_start[n] included.
 *                 -2  more than pcap distinct (small, stable) neighbour pairs.  Nothing else of that frame is touched either.
 *   The output carries no run_region: merged runs can join what were two regions.  The caller labels it with arseg_rle_regions_fwd.
 *   min_area == 1: every region is stable, the output code equals the input code, target is all -1 and n_absorbed 0.
 * workspace: the caller's, 8-byte aligned, >= arseg_rle_absorb_workspace_bytes(N, cap, rcap, H, pcap) bytes (else ARSEG_EWORKSPACE): per
 *   frame an open addressed table of pcap slots for the pairs (a 64-bit key and a 64-bit border), one 64-bit word per region record and a
 *   flag.  Probing visits every slot before it gives up, so an insert fails if and only if the frame has more than pcap distinct pairs: -2
 *   does not depend on timing.  A frame's distinct neighbouring run pairs are at most 3 x row_start[n][H] (runs - H in the rows, fewer
 *   than 2 x runs between rows), so pcap = 3 x cap can never give -2.  Its contents are scratch.
 * Six launches (clear + classify, vote, resolve, count, scan, emit); nothing is written into an output before the vote is known to have
 *   fitted; no workgroup waits for another.  Enqueue only: no allocation, no synchronisation.  The buffers must not overlap.
 * Malformed input (a run_region outside [0, R), a row_start that does not rise, x_first out of order) gives a meaningless code, but nothing
 *   outside the caller's buffers is read or written: indices and columns are clamped as arseg_rle_regions_fwd clamps them, and every loop
 *   is bounded.
 * ARSEG_EINVAL, before any launch: a null row_start, runs, n_regions, run_region, regions, out_row_start, out_runs or n_absorbed; one of
 *   them (regions apart) or target not 4-byte aligned; regions or the workspace not 8-byte aligned; non-positive N, H, W, cap, pcap or
 *   out_cap; min_area < 1; negative rcap or tcap; target == NULL with tcap > 0; W > 1 << 24; H * W > INT32_MAX; a null workspace.
 * Not covered: cascaded absorption inside one call; criteria other than the area (confidence, shape); filling holes only; morphological
 *   opening or closing; region or track ids carried across the rewrite; the pass fused into the run coder.
 * ------------------------------------------------------------------------------------------- */
size_t arseg_rle_absorb_workspace_bytes(int N, int64_t cap, int64_t rcap, int H, int64_t pcap);
int arseg_rle_absorb_fwd(const int32_t *row_start, const uint32_t *runs, const int32_t *n_regions, const int32_t *run_region, int64_t cap,
                         const int64_t *regions, int64_t rcap, int N, int H, int W, int64_t min_area, const uint8_t *protect,
                         int32_t *out_row_start, uint32_t *out_runs, int64_t out_cap, int32_t *target, int64_t tcap, int32_t *n_absorbed,
                         int64_t pcap, void *workspace, size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Region outlines as polygon loops (csrc/contours.hip): the shape of every region as closed loops of grid corners -- what an annotation
 * tool, a geo or CAD layer, a browser overlay or a shape matcher takes -- traced on the device from the run code alone (its run ends are
 * the vertical boundary segments of the mask; the plane is not read), without a host synchronisation: capturable in a HIP graph behind
 * arseg_rle_regions_fwd.
 * Input: row_start int32 [N][H+1], runs uint32 [N][cap], n_regions int32 [N] and run_region int32 [N][cap] exactly as
 *   arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them; the same N, H, W and cap; connectivity: the value the regions were labelled
 *   with (4 or 8).
 * Geometry.  Pixel (x, y) is the unit square [x, x+1] x [y, y+1].  A vertex is a grid corner (x, y), 0 <= x <= W, 0 <= y <= H, stored as
 *   the word y << 16 | x.  The boundary of region r is the set of unit edges between a pixel of r and a pixel that is not of r; the image
 *   border counts as a boundary.  Each edge is directed so that r lies on its right hand on the screen (y down): heading (hx, hy) has its
 *   right at (-hy, hx).  Outer loops therefore run clockwise on the screen and holes counter-clockwise.  At a vertex where r holds exactly
 *   two diagonal pixels (a saddle) the walk turns left when connectivity == 8 (the diagonal pixels are joined) and right when
 *   connectivity == 4; everywhere else the continuation is unique.  The edges of r fall into closed loops.  A loop is stored as its
 *   corners only: collinear vertices are dropped, so consecutive vertices differ in exactly one coordinate and the axes alternate.  A loop
 *   may pass through one vertex twice (a saddle).
 * Canonical form: the output is a pure function of the input.  A loop starts at its smallest vertex in (y, x) order (it is visited once).
 *   The loops of a frame are ordered by rising first vertex in (y, x) order; where two loops start at one vertex -- a hole and the outer
 *   loop of the region inside it -- the hole comes first.  In runs: every run has two vertical edges, 2 run + side with left end = 0 and
 *   right end = 1; the loops are ordered by their smallest edge, and a loop whose smallest edge is a right end is a hole.
 * Outputs, all integers, all OVERWRITTEN:
 *   counts      int32 [N][2] = {L, V}: the frame's loops and vertices, exact whatever lcap and vcap are (V below 2^31); or {-1, -1}: the
 *               frame cannot be processed -- row_start[n][H] > cap or n_regions[n] < 0 -- and nothing else of it is touched.  Decided on
 *               the device; nothing comes to the host.
 *   loops       int32 [N][lcap][4] = {region, first, count, hole}: first is the index of the loop's first vertex in the frame's list (the
 *               vertex counts of the loops before it), exact also when V > vcap.  The rows below min(L, lcap) are exact, the rows from
 *               there on untouched.  loops == NULL with lcap == 0: not wanted.
 *   verts       uint32 [N][vcap]: the vertices of the loops one after the other.  The words below min(V, vcap) are exact, the words from
 *               there on untouched.  verts == NULL with vcap == 0: not wanted (both: the sizing pass).
 *   The caller detects an overflow as L > lcap or V > vcap.  L <= row_start[n][H] (a loop has a smallest run end) and
 *   V <= 4 x row_start[n][H] (a run end gives at most two corners), so lcap = cap and vcap = 4 x cap never overflow.
 * workspace: the caller's, 4-byte aligned, >= arseg_rle_contours_workspace_bytes(N, cap) bytes (else ARSEG_EWORKSPACE): 80 bytes per run
 *   slot -- per run end its successor, the corner of its move and two states of the pointer jumping.  Its contents are scratch.
 * 4 + ceil(log2(2 cap)) launches (clear, successors, the jumps, scan, emit -- no emit without verts); the number is fixed by cap, so
 *   nothing comes back to the host; no workgroup waits for another.  Enqueue only: no allocation, no synchronisation.  The buffers must
 *   not overlap.
 * Malformed input (a row_start that does not rise, x_first out of order) gives meaningless loops, but nothing outside the caller's buffers
 *   is read or written: indices and columns are clamped as arseg_rle_regions_fwd clamps them, and every loop is bounded.
 * ARSEG_EINVAL, before any launch: a null row_start, runs, n_regions, run_region or counts; one of them, loops, verts or the workspace not
 *   4-byte aligned; non-positive N, H, W or cap; negative lcap or vcap; loops == NULL with lcap > 0, verts == NULL with vcap > 0;
 *   connectivity other than 4 or 8; H > 65535 or W > 65535 (the vertex word); cap > 1 << 29; a null workspace.
 * Not covered: smoothed polygons (splines; simplified ones: arseg_contours_simplify_fwd, further down); sub-pixel outlines from the
 *   logits; the nesting tree of holes and islands (a hole's region is given, the region inside it is the loop that follows it at the
 *   same vertex); outlines of absorbed masks in one call (label the output of arseg_rle_absorb_fwd and call again).
 * ------------------------------------------------------------------------------------------- */
size_t arseg_rle_contours_workspace_bytes(int N, int64_t cap);
int arseg_rle_contours_fwd(const int32_t *row_start, const uint32_t *runs, const int32_t *n_regions, const int32_t *run_region,
                           int64_t cap, int N, int H, int W, int connectivity, int32_t *counts, int32_t *loops, int64_t lcap,
                           uint32_t *verts, int64_t vcap, void *workspace, size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Region outlines simplified to a pixel tolerance (csrc/simplify.hip): the loops of arseg_rle_contours_fwd with the vertices dropped that
 * lie within a stated distance of the polygon that remains (Douglas-Peucker) -- what an overlay, an annotation tool or a tracker draws
 * instead of a vertex at every pixel step -- on the device, one more pass behind the outlines, without a host synchronisation:
 * capturable in the same HIP graph.  Integers only: every result is exact.  (A backward-compatible addition: ARSEG_ABI_VERSION stays.)
 * Input: counts int32 [N][2], loops int32 [N][lcap][4] and verts uint32 [N][vcap] exactly as arseg_rle_contours_fwd leaves them, with
 *   their capacities; H and W of the frames; tol2_q = 16 x the squared tolerance in pixels (0.5 px -> 4, 1 px -> 16, 1.5 px -> 36,
 *   2 px -> 64).
 * Rule per loop, on integer coordinates; the vertices are P[0 .. n) with P[n] = P[0]:
 *   1. Anchors.  a0 = 0 (the loop's smallest vertex: it is on the loop's hull); a1 = the position with the largest squared Euclidean
 *      distance from P[0], the smallest position of a tie.
 *   2. Chains.  Douglas-Peucker on the two open chains [a0, a1] and [a1, n].  For a segment (a, b) and its interior positions a < i < b,
 *      c_i = |(P[b] - P[a]) x (P[i] - P[a])|; the i with the largest c_i is picked, the smallest position of a tie.  If
 *      16 c_i^2 > tol2_q |P[b] - P[a]|^2 the vertex is kept and both halves are treated the same way; otherwise every interior vertex is
 *      dropped.  The distance is to the line through the two ends (as cv2.approxPolyDP measures it).  The ends of a segment never
 *      coincide: a1 is at positive distance from a0, and a kept vertex is strictly off its chord.
 *   3. No collapse.  If fewer than 3 vertices would be kept the loop is emitted unchanged, with all n vertices (a unit square stays a
 *      unit square).  Three kept vertices are never collinear, so every emitted loop is a proper polygon.
 *   4. Order.  Kept vertices keep their order, the loop still starts at the same first vertex; region and hole are copied; the loops keep
 *      their order.
 *   tol2_q = 0 gives the input back: an interior vertex of a corner loop is never on its chord.
 * Range: H, W <= 16384 keeps c_i <= 2^29 (32-bit products) and, with tol2_q <= 2^30, both sides of the comparison below 2^63.
 * Outputs, all integers, all OVERWRITTEN:
 *   counts_out  int32 [N][2] = {L, V'}: exact whatever vcap_out is; or {-1, -1}: the frame is refused -- its source counts are negative,
 *               or L > lcap or V > vcap (an overflowed source) -- and nothing else of it is touched.  Decided on the device.
 *   loops_out   int32 [N][lcap][4] = {region, first', count', hole}: first' is the prefix sum of count', exact also when V' > vcap_out.
 *               The rows below L are exact, the rows from there on untouched.
 *   verts_out   uint32 [N][vcap_out]: the words below min(V', vcap_out) are exact, the words from there on untouched.  verts_out == NULL
 *               with vcap_out == 0: the sizing pass.  V' <= V, so vcap_out = vcap never overflows.
 * workspace: the caller's, 4-byte aligned, >= arseg_contours_simplify_workspace_bytes(N, lcap, vcap) bytes (else ARSEG_EWORKSPACE): per
 *   frame 4 bytes per loop slot (the kept count) and a byte per vertex slot (the keep flag); capacities whose size does not fit size_t
 *   give SIZE_MAX and ARSEG_EWORKSPACE.  Its contents are scratch.
 * 4 launches (clear, keep, scan, emit -- no emit without verts_out), sized on the host from the capacities; no workgroup waits for
 *   another.  Enqueue only: no allocation, no synchronisation.  The buffers must not overlap.
 * Malformed input (a loop record whose first or count lies outside the frame's vertices) gives meaningless output, but nothing outside
 *   the caller's buffers is read or written: first and count are clamped into [0, min(V, vcap)], and every loop is bounded.
 * ARSEG_EINVAL, before any launch: a null counts or counts_out; loops or loops_out NULL with lcap > 0, verts NULL with vcap > 0,
 *   verts_out NULL with vcap_out > 0; one of the arrays or the workspace not 4-byte aligned; non-positive N, H or W; a negative
 *   capacity; H > 16384 or W > 16384; tol2_q < 0 or > 1 << 30; verts_out == verts, loops_out == loops or counts_out == counts; a null
 *   workspace.
 * Not covered: a border shared by two regions is simplified once per loop, so the two results may differ by up to the tolerance
 *   (arseg_contours_simplify_shared_fwd, below, cuts the loops where three regions meet and simplifies each arc once); smoothing;
 *   area-preserving rules.
 * ------------------------------------------------------------------------------------------- */
size_t arseg_contours_simplify_workspace_bytes(int N, int64_t lcap, int64_t vcap);
int arseg_contours_simplify_fwd(const int32_t *counts, const int32_t *loops, int64_t lcap, const uint32_t *verts, int64_t vcap, int N, int H,
                                int W, int64_t tol2_q, int32_t *counts_out, int32_t *loops_out, uint32_t *verts_out, int64_t vcap_out,
                                void *workspace, size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Region outlines simplified with shared borders (csrc/simplify_shared.hip): arseg_contours_simplify_fwd's output for consumers that lay
 * neighbouring polygons side by side -- a vector overlay, a GIS layer, an annotation tool --: a border between two regions is cut out of
 * both loops at the same points and simplified by a rule that does not depend on the direction of travel, so the two neighbours keep
 * the same vertices of it and no sliver or overlap opens between them.  On the device, behind arseg_rle_contours_fwd, without a host
 * synchronisation: capturable in the same HIP graph.  Integers only: every result is exact.  (A backward-compatible addition:
 * ARSEG_ABI_VERSION stays.)
 * Input: row_start int32 [N][H+1] and runs uint32 [N][cap] (the run code the outlines were traced from, as arseg_labels_rle_fwd or
 *   arseg_rle_absorb_fwd leaves it); counts int32 [N][2], loops int32 [N][lcap][4] and verts uint32 [N][vcap] exactly as
 *   arseg_rle_contours_fwd leaves them, with their capacities; H and W of the frames; tol2_q = 16 x the squared tolerance in pixels.
 * Junctions.  Four unit grid edges meet at a grid corner (x, y), each between two of its four pixels.  A grid edge is a border edge if
 *   its two pixels differ in value, or if exactly one of them lies outside the frame (side-adjacent pixels of one value are one region
 *   at either connectivity, so the values decide).  The degree of a corner is its number of border edges: 0, 2, 3 or 4.  A corner is a
 *   junction if its degree is at least 3, or if it is one of the four corners of the frame (else the corners of the picture would be
 *   cut off).  A saddle has degree 4: a junction at either connectivity.
 * Expanded loop.  The source loop (corners only) plus, on each of its straight edges, every junction strictly inside that edge, in
 *   travel order: the T-junctions whose straight side is this loop -- the two regions on the other side have a corner there.  Every
 *   vertex of the expanded loop is a junction passage or an ordinary corner; a loop may pass one junction twice (a saddle), and each
 *   passage counts.
 * Arcs.  The expanded loop is cut at every junction passage; an arc runs from one passage to the next, cyclically.  A loop without a
 *   junction is one closed arc from the source loop's first vertex; a loop with one passage is one closed arc from that passage round to
 *   itself; two different passages may be the same point (a one-pixel appendage on a saddle), and the arc between them is closed too.
 *   Inside an arc every vertex has degree 2: an arc never visits a point twice and has the same two regions on its two sides all along.
 * Rule per arc, on integer coordinates; the arc's points are P[0 .. m]:
 *   open (P[0] != P[m]): both ends are kept; Douglas-Peucker on (0, m) as in arseg_contours_simplify_fwd's rule 2 -- c_i = |(P[b] - P[a])
 *     x (P[i] - P[a])|, the largest c_i picked, kept with both halves treated the same way iff 16 c_i^2 > tol2_q |P[b] - P[a]|^2 -- with
 *     one change: among ties the SMALLEST VERTEX WORD is picked, not the smallest position.  That makes the rule the same in both
 *     directions of travel.
 *   closed (P[0] == P[m]): P[0] is kept; a1 = the position in [0, m) with the largest squared distance from P[0], the smallest vertex
 *     word of a tie, is kept; Douglas-Peucker on (0, a1) and (a1, m).  If fewer than 3 vertices would be kept all m are kept (the arc's
 *     other side decides the same: a one-pixel island and its hole both stay squares).
 * Outputs, all integers, all OVERWRITTEN, in the format and order of arseg_contours_simplify_fwd:
 *   counts_out  int32 [N][2] = {L, V'}: exact whatever vcap_out is; or {-1, -1}: the frame is refused -- its source counts are negative,
 *               L > lcap, V > vcap or row_start[n][H] > cap -- and nothing else of it is touched.  Decided on the device.
 *   loops_out   int32 [N][lcap][4] = {region, first', count', hole}: first' is the prefix sum of count', exact also when V' > vcap_out;
 *               region and hole are copied, the loops keep their order.  The rows below L are exact, the rows from there on untouched.
 *   verts_out   uint32 [N][vcap_out]: a loop's kept vertices in source order, from the first kept position at or after the source
 *               loop's first vertex.  The words below min(V', vcap_out) are exact, the words from there on untouched.  verts_out ==
 *               NULL with vcap_out == 0: the sizing pass.
 *   tol2_q = 0 gives the expanded loops: the source corners plus the inserted junctions.
 *   V' can exceed V: at most one vertex is inserted per end of an interior vertical unit border edge whose junction has a straight
 *   side, and there are row_start[n][H] - H such edges, so V' <= V + 2 x row_start[n][H] and vcap_out = vcap + 2 x cap never overflows.
 *   Degenerate loops are emitted as they are: a loop made of open arcs that all collapse onto their chords comes out with count' = 2
 *   or with collinear vertices -- its region is thinner than the tolerance, its neighbours close over it without a gap, and restoring it
 *   would break the match with them.  count' >= 2 always.
 * workspace: the caller's, 4-byte aligned, >= arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap) bytes (else
 *   ARSEG_EWORKSPACE): per frame 12 bytes per loop slot, 4 per vertex slot and 5 per slot of the expanded loops (vcap + 2 cap of
 *   them); capacities whose size does not fit size_t give SIZE_MAX and ARSEG_EWORKSPACE.  Its contents are scratch.
 * 7 launches (mark, place, scan, expand, keep, scan, emit -- no emit without verts_out), sized on the host from the capacities; no workgroup
 *   waits for another.  Enqueue only: no allocation, no synchronisation.  The buffers must not overlap.
 * Malformed input (a run code or loop records that do not belong together) gives meaningless output, but nothing outside the caller's
 *   buffers is read or written: rows, run indices, loop records and expanded slots are clamped, and every loop is bounded.
 * ARSEG_EINVAL, before any launch: a null row_start, runs, counts or counts_out; loops or loops_out NULL with lcap > 0, verts NULL with
 *   vcap > 0, verts_out NULL with vcap_out > 0; one of the arrays or the workspace not 4-byte aligned; non-positive N, H, W or cap; a
 *   negative lcap, vcap or vcap_out; H > 16384 or W > 16384; tol2_q < 0 or > 1 << 30; cap > 1 << 29; an output that is one of the
 *   inputs; a null workspace.
 * Not covered: the arcs themselves as output (shared arcs with per-loop arc lists); self-intersection repair; smoothing and
 *   area-preserving rules; more than one wave per long loop.
 * ------------------------------------------------------------------------------------------- */
size_t arseg_contours_simplify_shared_workspace_bytes(int N, int64_t cap, int64_t lcap, int64_t vcap);
int arseg_contours_simplify_shared_fwd(const int32_t *row_start, const uint32_t *runs, int64_t cap, const int32_t *counts,
                                       const int32_t *loops, int64_t lcap, const uint32_t *verts, int64_t vcap, int N, int H, int W,
                                       int64_t tol2_q, int32_t *counts_out, int32_t *loops_out, uint32_t *verts_out, int64_t vcap_out,
                                       void *workspace, size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Region polygons rasterised back to a label plane, with the fidelity counters (csrc/fill.hip): the inverse and the check of the three
 * passes above -- the mask a consumer of the polygons draws, and what the simplification did to it: uncovered pixels, doubly covered
 * pixels, pixels that changed value, and per value the areas and the intersection with the mask the outlines were traced from.  On the
 * device, behind the passes above, without a host synchronisation: capturable in the same HIP graph.  Integers only: every result is
 * exact and reproducible.  (A backward-compatible addition: ARSEG_ABI_VERSION stays.)
 * Input, per frame: counts int32 [N][2], loops int32 [N][lcap][4] and verts uint32 [N][vcap] exactly as arseg_rle_contours_fwd,
 *   arseg_contours_simplify_fwd or arseg_contours_simplify_shared_fwd leave them, with their capacities; n_regions int32 [N] and records
 *   int64 [N][rcap][8] of arseg_rle_regions_fwd, of which only records[n][r][0], the region's value (its low byte), is read; H and W of
 *   the frames, at most 16384; background, a byte; optionally ref_labels uint8 with ref_pitch and ref_image_stride (bytes): the mask the
 *   outlines were traced from.
 * Crossing.  Vertices are grid corners; the centre of pixel (x, y) is (x + 1/2, y + 1/2), so a pixel row never passes through a vertex.
 *   An edge A -> B with ya != yb crosses the rows min(ya, yb) <= y < max(ya, yb); horizontal edges cross nothing.  Order the edge so that
 *   ya < yb, whatever its direction of travel; with dy = yb - ya and t = 2 y + 1 - 2 ya the crossing column is
 *       xs = ceil((2 xa dy + t (xb - xa) - dy) / (2 dy)),
 *   the first column whose centre lies at or to the right of the edge, clamped into [0, W]; floor and ceiling are those of a negative
 *   numerator too; all terms stay below 2^31 for H, W <= 16384.  A centre exactly on an edge therefore belongs to the polygon on the
 *   right of the edge, and two loops that share an edge compute the same xs: the formula does not depend on the direction of travel.
 * Coverage (even-odd per region).  For region r and row y sort the crossings of all edges of all loops whose record names r:
 *   c0 <= c1 <= ... -- always an even number --; r covers the columns [c0, c1) u [c2, c3) u ...  The orientation of the loops and their
 *   hole flag are not read.  A two-vertex loop, which arseg_contours_simplify_shared_fwd can emit, cancels itself.
 * Composition (painter's rule).  A pixel covered by k regions takes the value of the covering region with the largest region number; a
 *   pixel with k = 0 takes background.  That equals filling each region's loops in rising region number over a plane of background --
 *   what a consumer does with fillPoly-style calls.
 * Outputs, all OVERWRITTEN:
 *   labels_out  uint8, row y of frame n at labels_out + n * image_stride + y * pitch.
 *   counts_out  int32 [N]: E, the number of crossings the frame needs, exact whatever ecap is (INT32_MAX from there on); or -1: the frame
 *               is refused -- its source counts are negative, L > lcap, V > vcap, n_regions[n] < 0 or n_regions[n] > rcap -- and nothing
 *               else of it is touched.  A frame with E > ecap gets its counts_out and nothing else.  Decided on the device.
 *   stats       int64 [N][ARSEG_FILL_NSTATS] = {gaps, excess, changed, ref_area[256], fill_area[256], both[256]} (may be NULL): gaps the
 *               pixels with k = 0; excess the sum of max(k - 1, 0) over the pixels; changed the pixels whose output differs from
 *               ref_labels, gap pixels counting as changed; ref_area[v] the pixels of value v in the reference; fill_area[v] the covered
 *               pixels that received v; both[v] the covered pixels with v in both.  Without a reference changed, ref_area and both are 0.
 *   labels_out == NULL with ecap == 0: the sizing pass, counts_out only.
 * Capacity.  The loops of arseg_rle_contours_fwd, arseg_contours_simplify_fwd and arseg_contours_simplify_shared_fwd that come from a
 *   run code of capacity cap need E <= 2 x cap: the exact outlines have 2 x runs unit crossings (a run's two ends), and a Douglas-Peucker
 *   chord never spans more rows than the chain it replaces.  ecap = 2 x cap therefore never overflows for them.
 * workspace: the caller's, 8-byte aligned, >= arseg_contours_fill_workspace_bytes(N, H, W, lcap, vcap, ecap) bytes (else
 *   ARSEG_EWORKSPACE): per frame 8 bytes per crossing slot and 8 per row and one more, and for W > 8192 one owner line of 4 W bytes per
 *   workgroup of the row launch (at most 256); sizes that do not fit size_t give SIZE_MAX and ARSEG_EWORKSPACE.  Its contents are scratch.
 * 5 launches (clear, count, scan, scatter, rows -- the first three in a sizing pass), sized on the host from the capacities; no workgroup
 *   waits for another.  Enqueue only: no allocation, no synchronisation.  The buffers must not overlap.  A row with m crossings costs
 *   m x m comparisons (a rank by counting), on chip up to 1024 crossings and from L2 beyond.
 * Malformed input (a loop outside the frame's vertices, a region number outside [0, n_regions), a vertex beyond W or H) gives
 *   meaningless output, but nothing outside the caller's buffers is read or written: loop records, region numbers, vertices, bucket
 *   bounds and slots are clamped, and every loop is bounded.
 * ARSEG_EINVAL, before any launch: a null counts, n_regions or counts_out; loops NULL with lcap > 0, verts NULL with vcap > 0, records
 *   NULL with rcap > 0, labels_out NULL with ecap > 0; counts, loops, verts, n_regions or counts_out not 4-byte aligned, records, stats
 *   or the workspace not 8-byte aligned; non-positive N, H or W; H > 16384 or W > 16384; a negative capacity; background outside
 *   0..255; pitch < W or ref_pitch < W, a negative image stride; an output that is one of the inputs or another output; a null workspace.
 * Not covered: anti-aliased (fractional) coverage; non-integer vertices; winding-rule fills; frames of more than 16384 rows or columns.
 * ------------------------------------------------------------------------------------------- */
#define ARSEG_FILL_NSTATS (3 + 3 * 256)
size_t arseg_contours_fill_workspace_bytes(int N, int H, int W, int64_t lcap, int64_t vcap, int64_t ecap);
int arseg_contours_fill_fwd(const int32_t *counts, const int32_t *loops, int64_t lcap, const uint32_t *verts, int64_t vcap,
                            const int32_t *n_regions, const int64_t *records, int64_t rcap, int N, int H, int W, int background,
                            const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, uint8_t *labels_out, int64_t pitch,
                            int64_t image_stride, int32_t *counts_out, int64_t *stats, int64_t ecap, void *workspace,
                            size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Confusion counts in bands around the label boundaries (csrc/bands.hip): where the errors are, next to the evaluator tail's how many --
 * the "trimap" accuracy of DeepLab, the band Boundary IoU is built on.  No reference counterpart.
 * Void.      label is int64 [N][H][W], contiguous, as the evaluator tail takes it.  Every pixel becomes a byte: v = label if
 *            0 <= label < n_cls and label != ignore_label, else 255 ("void").  All void pixels are one value.
 * Distance.  D(p) is the smallest r >= 1 such that the (2r+1) x (2r+1) window centred at p, CLIPPED to the image, holds a pixel whose
 *            byte differs from p's: a Chebyshev distance, what r iterations of a 3 x 3 erosion remove.  The image border is not a
 *            boundary; a frame of one value has none.
 * Bands.     radii is a HOST array of n_bands ints, strictly ascending, 1 <= radii[k] <= 32, 1 <= n_bands <= 8.  band(p) is the smallest
 *            k with D(p) <= radii[k], and n_bands ("interior") if D(p) > radii[n_bands - 1].  The bands are disjoint; cumulating them
 *            (a trimap of width radii[k] is the bands 0 .. k) is the host's business.
 * Tally.     pred is int32 [N][H][W], what arseg_argmax_confusion*_fwd write; group is int32 [N] on the device and may be NULL only
 *            when n_groups == 1: every frame is then group 0.  Every non-void pixel with 0 <= pred < n_cls, in a frame whose group id is
 *            in [0, n_groups), adds 1 to hist[group[n]][band(p)][label][pred]; hist is int64 [n_groups][n_bands + 1][n_cls][n_cls],
 *            ACCUMULATED.  Void pixels count nowhere; they still get a band and still are a boundary for their neighbours, as the void
 *            ring of a VOC-style annotation is.  The sum of hist[g] over the bands is bit-equal to the hist[g] that
 *            arseg_argmax_confusion_grouped_fwd gives on the same labels and the logits the predictions come from.
 * band_out   uint8, band(p) of row y of frame n at band_out + n * band_n_stride + y * band_pitch (bytes; band_pitch >= W,
 *            band_n_stride >= 0); OVERWRITTEN, for every frame and pixel, void ones included.  May be NULL.
 * pred and hist may be NULL together (the bands of a plane only); pred without hist is not read.  With band_out and hist both NULL only
 *            the first launch runs, which leaves the workspace's words (tools/bench_bands.py times the launches apart that way).
 * workspace: the caller's, 2-byte aligned, >= arseg_label_bands_workspace_bytes(N, H, W) bytes (else ARSEG_EWORKSPACE): one 16-bit word
 *            per pixel, rounded up to 16 bytes in all (0 for dimensions the entry point refuses; a size that does not fit size_t gives
 *            SIZE_MAX).  Its contents are scratch.
 * 2 launches (rows: label -> byte and in-row distance; columns: the distance, the band, the tally), sized on the host; no workgroup
 *            waits for another.  Enqueue only: no allocation, no synchronisation; capturable in a HIP graph.  The buffers must not
 *            overlap.
 * Malformed labels only ever give void, predictions outside [0, n_cls) and group ids outside [0, n_groups) count nowhere; nothing
 *            outside the caller's buffers is read or written, and every loop is bounded.
 * ARSEG_EINVAL, before any launch: a null label, radii or workspace; non-positive N, H or W; H > 16384 or W > 16384; n_bands outside
 *            1..8, a radius outside 1..32 or radii that do not ascend strictly; n_cls outside 1..32; n_groups < 1; a null group with
 *            n_groups > 1; hist without pred; with band_out, band_pitch < W or a negative band_n_stride; label or hist not 8-byte
 *            aligned, pred or group not 4-byte aligned, the workspace not 2-byte aligned.
 * Not covered: Euclidean distance.  Boundary IoU proper, radii above 32 and the image border as a boundary are the next entry point's.
 * ------------------------------------------------------------------------------------------- */
size_t arseg_label_bands_workspace_bytes(int N, int H, int W);
int arseg_label_bands_fwd(const int64_t *label, const int32_t *pred, const int32_t *group, const int *radii, int n_bands, uint8_t *band_out,
                          int64_t band_pitch, int64_t band_n_stride, int64_t *hist, int N, int n_groups, int n_cls, int H, int W,
                          int ignore_label, void *workspace, size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Boundary IoU counts from joint label / prediction bands (csrc/bands.hip; Cheng et al., "Boundary IoU", CVPR 2021): per class the
 * inner boundary band of the ground-truth mask, that of the predicted mask, and their intersection, in disjoint bands of width.  No
 * reference counterpart.
 * Bytes.     label is int64 [N][H][W], pred int32 [N][H][W], both contiguous and both required.  A label becomes a byte exactly as in
 *            arseg_label_bands_fwd (itself if 0 <= label < n_cls and label != ignore_label, else 255); a prediction becomes a byte:
 *            itself if 0 <= pred < n_cls, else 255.  Each plane's bytes alone decide that plane's distances.
 * Distance.  D(p) on a byte plane is arseg_label_bands_fwd's Chebyshev distance: the smallest r >= 1 whose (2r+1) x (2r+1) window at
 *            p, clipped to the image, holds another byte.  With border != 0, D(p) is also at most min(x + 1, y + 1, W - x, H - y), the
 *            smallest r whose window leaves the image: the image border is a boundary, as under the zero-padded erosion of the
 *            published implementation.  With border == 0, D on the label plane is arseg_label_bands_fwd's, bit for bit.
 * Bands.     radii is a HOST array of n_bands ints, strictly ascending, 1 <= radii[k] <= 64, 1 <= n_bands <= 8.  band(p) is the smallest
 *            k with D(p) <= radii[k], and n_bands for the interior; bg is the band on the label plane, bp that on the prediction plane.
 * Counts.    group as in arseg_label_bands_fwd (int32 [N] on the device; NULL only with n_groups == 1).  A pixel counts if its label
 *            byte is not 255, its prediction byte is not 255 and its frame's group id g is in [0, n_groups).  counts is int64
 *            [n_groups][3][n_bands + 1][n_cls], ACCUMULATED; a counting pixel adds 1 to counts[g][0][bg][label] and to
 *            counts[g][1][bp][pred], and, if label == pred, to counts[g][2][max(bg, bp)][label].  Void-labelled pixels count nowhere
 *            and are a boundary for their neighbours on the label plane, as predictions outside the classes are on theirs.  The bands
 *            are disjoint; cumulating them is the host's business: at radii[k], with I, G and P the sums over the bands 0 .. k of rows
 *            2, 0 and 1, the Boundary IoU of class c is I / (G + P - I).  Summed over all n_bands + 1 bands, rows 0, 1 and 2 are the
 *            row sums, column sums and diagonal of arseg_argmax_confusion_grouped_fwd's hist on the same inputs, exactly.
 * label_band_out, pred_band_out: uint8, bg and bp of row y of frame n at out + n * n_stride + y * pitch (bytes; pitch >= W,
 *            n_stride >= 0); OVERWRITTEN, for every frame and pixel.  Each may be NULL; counts may be NULL if a plane is given.
 * workspace: the caller's, 2-byte aligned, >= arseg_boundary_iou_workspace_bytes(N, H, W) bytes (else ARSEG_EWORKSPACE): two 16-bit
 *            words per pixel, 4 N H W bytes rounded up to 16 (0 for dimensions the entry point refuses; a size that does not fit
 *            size_t gives SIZE_MAX).  Its contents are scratch.
 * 2 launches (rows: both planes' bytes and in-row distances; columns: the distances, the bands, the tally), sized on the host; no
 *            workgroup waits for another.  Enqueue only: no allocation, no synchronisation; capturable in a HIP graph.  The buffers
 *            must not overlap.  Malformed labels and predictions only ever give the byte 255; nothing outside the caller's buffers is
 *            read or written, and every loop is bounded.
 * ARSEG_EINVAL, before any launch and before ARSEG_EWORKSPACE: a null label, pred, radii or workspace; non-positive N, H or W; H > 16384
 *            or W > 16384; n_bands outside 1..8, a radius outside 1..64 or radii that do not ascend strictly; n_cls outside 1..32;
 *            n_groups < 1; a null group with n_groups > 1; border outside {0, 1}; all three outputs null; with a plane, its pitch < W
 *            or a negative n_stride; label or counts not 8-byte aligned, pred or group not 4-byte aligned, the workspace not 2-byte
 *            aligned.
 * Not covered: Euclidean distance; radii above 64; Boundary AP / PQ; min(IoU, Boundary IoU); fusion into the argmax launch.
 * ------------------------------------------------------------------------------------------- */
size_t arseg_boundary_iou_workspace_bytes(int N, int H, int W);
int arseg_boundary_iou_fwd(const int64_t *label, const int32_t *pred, const int32_t *group, const int *radii, int n_bands, int border,
                           uint8_t *label_band_out, int64_t label_band_pitch, int64_t label_band_n_stride, uint8_t *pred_band_out,
                           int64_t pred_band_pitch, int64_t pred_band_n_stride, int64_t *counts, int N, int n_groups, int n_cls, int H,
                           int W, int ignore_label, void *workspace, size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Contour F-measure counts from matched class contours (csrc/bands.hip): per class the contour pixels of the ground truth and of the
 * prediction, by the distance to the nearest contour pixel of the same class on the other plane -- the precision and recall of the
 * contours within a pixel tolerance, the F of the DAVIS protocol's "J & F" and the BF score of Csurka et al. (Matlab's bfscore).  No
 * reference counterpart.
 * Bytes.     label is int64 [N][H][W], pred int32 [N][H][W], both contiguous and both required.  Labels and predictions become bytes
 *            exactly as in the entry point above: a label is itself if 0 <= label < n_cls and label != ignore_label, else 255; a
 *            prediction is itself if 0 <= pred < n_cls, else 255.  1 <= n_cls <= 32.
 * Contours.  On either byte plane a pixel with byte c != 255 is a contour pixel of class c exactly when one of its 8 neighbours INSIDE the
 *            image has a byte that is neither c nor 255: the inner contour of each class mask.  The image border is no contour, and a
 *            255 neighbour makes none: void areas hide the true contour, they are not evidence of one.  On a plane without 255 these
 *            are the pixels with D(p) == 1 of arseg_label_bands_fwd.
 * Match.     For a contour pixel p of class c on one plane, m2(p) is the smallest dx^2 + dy^2 to a contour pixel of class c on the OTHER
 *            plane of the same frame: 0 if the other plane has one at p itself, infinite if it has none.  radii is a HOST array of
 *            n_bands ints, strictly ascending, 0 <= radii[k] <= 32, 1 <= n_bands <= 8.  band(p) is the smallest k with
 *            m2(p) <= radii[k]^2, and n_bands if there is none ("unmatched").  The tolerance is a disc, as DAVIS's dilation and
 *            bfscore's distance threshold are, not the square of the two entry points above.  All arithmetic is integer.
 * Counts.    group as in the entry points above (int32 [N] on the device; NULL only with n_groups == 1).  A pixel counts if neither of
 *            its two bytes is 255 and its frame's group id g is in [0, n_groups).  counts is int64 [n_groups][2][n_bands + 1][n_cls],
 *            ACCUMULATED; a counting contour pixel of class c of the label plane adds 1 to counts[g][0][band(p)][c], one of the
 *            prediction plane to counts[g][1][band(p)][c].  Contour pixels that do not count are still match targets for the other
 *            plane.  The bands are disjoint; cumulating them is the host's business: at radii[k] the recall of class c is row 0
 *            summed over the bands 0 .. k divided by row 0 summed over all n_bands + 1 bands, the precision the same on row 1, and
 *            F = 2 P R / (P + R).
 * label_match_out, pred_match_out: uint8, row y of frame n at out + n * n_stride + y * pitch (bytes; pitch >= W, n_stride >= 0);
 *            OVERWRITTEN, for every frame and pixel: band(p) at every contour pixel of that plane, counting or not, 255 elsewhere.
 *            Each may be NULL; counts may be NULL if a plane is given.
 * workspace: the caller's, 2-byte aligned, >= arseg_contour_f_workspace_bytes(N, H, W) bytes (else ARSEG_EWORKSPACE): one byte per pixel
 *            and plane, 2 N H W bytes rounded up to 16 (0 for dimensions the entry point refuses; a size that does not fit size_t
 *            gives SIZE_MAX).  Its contents are scratch.
 * 2 launches (marks: both planes' bytes and their 3 x 3 contour test; match: the search, the bands, the tally), sized on the host; no
 *            workgroup waits for another.  Enqueue only: no allocation, no synchronisation; capturable in a HIP graph.  The buffers
 *            must not overlap.  Malformed labels and predictions only ever give the byte 255; nothing outside the caller's buffers is
 *            read or written, and every loop is bounded.
 * ARSEG_EINVAL, before any launch and before ARSEG_EWORKSPACE: a null label, pred, radii or workspace; non-positive N, H or W; H > 16384
 *            or W > 16384; n_bands outside 1..8, a radius outside 0..32 or radii that do not ascend strictly; n_cls outside 1..32;
 *            n_groups < 1; a null group with n_groups > 1; all three outputs null; with a plane, its pitch < W or a negative n_stride;
 *            label or counts not 8-byte aligned, pred or group not 4-byte aligned, the workspace not 2-byte aligned.
 * Not covered: the both-sided contour of DAVIS's seg2bmap; one-to-one (bipartite) matching as in BSDS; the mean of per-frame F (the
 *            counts are pooled per group; one group per frame gives it); a void neighbour or the image border as a contour; radii
 *            above 32; the Chebyshev tolerance.
 * ------------------------------------------------------------------------------------------- */
size_t arseg_contour_f_workspace_bytes(int N, int H, int W);
int arseg_contour_f_fwd(const int64_t *label, const int32_t *pred, const int32_t *group, const int *radii, int n_bands,
                        uint8_t *label_match_out, int64_t label_match_pitch, int64_t label_match_n_stride, uint8_t *pred_match_out,
                        int64_t pred_match_pitch, int64_t pred_match_n_stride, int64_t *counts, int N, int n_groups, int n_cls, int H,
                        int W, int ignore_label, void *workspace, size_t workspace_bytes, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Calibration counts (csrc/calibration.hip): the reliability table of the confidence code -- per group of frames (keyframe distance),
 * predicted class and 8-bit code how many pixels there were and how many of them were right -- from the logits and the ground truth in
 * one launch for N frames and one pass over the logits; neither resized logits, probabilities nor the two byte planes exist.  ECE, MCE,
 * class-wise ECE, risk-coverage and the threshold for a target precision are host arithmetic on these integers
 * (arseg_amd.evaluation.CalibrationTable).  No reference counterpart.
 * Logits.    logits, N, n_cls, h, w, H, W, align_corners, kind: exactly as arseg_segment_confidence_fwd takes them, with its route choice
 *            (h == H && w == W; per-pixel bilinear, either align_corners; the x2 / x4 / x8 align_corners == 0 run route with its first and
 *            last half runs).  The class k* and the code q of an output pixel come from the one label rule (csrc/arseg_device.h) with the
 *            softmax accumulator of the confidence launch: they are bit-equal to labels8 (identity lut) and conf8 of
 *            arseg_segment_confidence_fwd on the same arguments; a pixel whose confidence is NaN has q = 0.  1 <= n_cls <= 32.
 * Labels.    label is int64 [N][H][W], contiguous.  A pixel counts if 0 <= label < n_cls and label != ignore_label (the tail's rule).
 * Groups.    group is int32 [N] on the device, NULL only with n_groups == 1 (every frame is then group 0).  A frame whose group id is
 *            outside [0, n_groups) counts nowhere.
 * Counts.    cal is int64 [n_groups][n_cls][256][2], ACCUMULATED.  A counting pixel of a frame of group g adds 1 to cal[g][k*][q][0], and 1
 *            to cal[g][k*][q][1] if label == k*.  Integers only: independent of the order of the atomic adds, so two runs are bit-equal.
 *            Summing over the classes (the usual reliability diagram) is the host's business.
 * Link to the tail.  On the same logits, labels and groups, with hist of arseg_argmax_confusion_grouped_fwd (hist[g][label][pred]):
 *              sum_q cal[g][k][q][0] == sum_l hist[g][l][k]        (column k: the pixels predicted k)
 *              sum_q cal[g][k][q][1] == hist[g][k][k]              (the diagonal: the pixels predicted k that are k)
 *            exactly.
 * Enqueue only: no allocation, no synchronisation, no workspace; capturable in a HIP graph.  cal must not overlap the inputs.
 * ARSEG_EINVAL, before any launch: null logits, label or cal; a null group with n_groups > 1; n_groups < 1; n_cls outside 1..32; a
 *            non-positive size; an unknown kind; label or cal not 8-byte aligned; group not 4-byte aligned.
 * Not covered: NLL / Brier score (float sums); entropy; the confusion matrix from the same launch (arseg_argmax_confusion_grouped_fwd
 *            keeps it); temperature fitting.
 * ------------------------------------------------------------------------------------------- */
int arseg_calibration_fwd(const float *logits, const int64_t *label, const int32_t *group, int64_t *cal, int N, int n_groups, int n_cls,
                          int h, int w, int H, int W, int ignore_label, int align_corners, int kind, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement aids (no reference counterpart; BASELINE.md section 3: roofline fractions are reported against the datasheet peaks AND
 * against on-box micro-benchmarks).  bench.py times each with HIP events and prints `peaks_measured`.
 *   arseg_peak_stream_copy: dst[0 .. n_bytes) = src[0 .. n_bytes) with 16-byte accesses (n_bytes % 16 == 0, both 16-byte aligned):
 *                           2 x n_bytes of HBM traffic per launch.
 *   arseg_peak_mfma_f16:    a full-chip launch whose every wave issues iters x 8 independent v_mfma_f32_32x32x16_f16 and touches no
 *                           memory (scratch: >= 4 bytes, never written in practice); *flops_out (may be NULL) = FLOPs issued per launch.
 * ------------------------------------------------------------------------------------------- */
int arseg_peak_stream_copy(const void *src, void *dst, size_t n_bytes, arseg_stream_t stream);
int arseg_peak_mfma_f16(float *scratch, int iters, double *flops_out, arseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The symbol names SURVEY.md section 8(b) lists for this boundary, as aliases of the entry points above (identical arguments):
 *   arseg_creff_fused_fwd     = arseg_creff_warp_fwd      (warp + CReFF + final 1x1 in one launch)
 *   arseg_conv2d_bn_act_fwd   = arseg_conv2d_fwd          arseg_pack_weights      = arseg_pack_conv_weight_host
 *   arseg_maxpool3x3s2        = arseg_maxpool3x3s2_fwd    arseg_adaptive_avgpool  = arseg_adaptive_avgpool_fwd
 *   arseg_global_reduce       = arseg_global_reduce_fwd   arseg_resize            = arseg_resize_fwd
 *   arseg_scale_add           = arseg_scale_add_fwd
 * ------------------------------------------------------------------------------------------- */
int arseg_creff_fused_fwd(const float *const *ref_nhwc_host, const int16_t *mv_q, int H, int W, const float *lr, const float *wq,
                          const float *bq, const float *wk, const float *bk, const float *wv, const float *bv, float *p_out, int p_layout,
                          const float *wf, const float *bf, int n_cls, float *logits, int log_softmax, int N, int C, int Hp, int Wp, int hp,
                          int wp, int kH, int kW, arseg_stream_t stream);
int arseg_conv2d_bn_act_fwd(const arseg_conv_desc *d, const float *in, const float *w_packed, const float *scale, const float *bias,
                            const float *residual, float *out, void *workspace, size_t workspace_bytes, arseg_stream_t stream);
int arseg_pack_weights(const float *w_oihw_host, int Cout, int Cin, int R, int S, int Cin_pad, float *out_host);
int arseg_maxpool3x3s2(const float *in, float *out, int N, int H, int W, int C, arseg_stream_t stream);
int arseg_adaptive_avgpool(const float *in, int in_ld, float *out, int out_ld, long long out_n_stride, int N, int H, int W, int C, int oh,
                           int ow, arseg_stream_t stream);
int arseg_global_reduce(const float *in, int in_ld, float *out, int N, int H, int W, int C, int op, arseg_stream_t stream);
int arseg_resize(const float *in, float *out, int N, int C, int Hin, int Win, int Hout, int Wout, int mode, int align_corners, int layout,
                 int in_ld, int out_ld, arseg_stream_t stream);
int arseg_scale_add(const float *x, const float *scale, const float *add_full, const float *add_vec, float *out, int N, int HW, int C,
                    arseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ARSEG_HIP_H */
